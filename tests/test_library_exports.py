"""CPU-side checks of the product library: it loads, exports every symbol of include/graphchainer_amd.h, and
fails loudly (no fallback) when no GPU is present."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import graphchainer_amd as gca
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return gca.load_library()


def test_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "graphchainer_amd.h")).read()
    declared = set(re.findall(r"\b(gc_[a-z_]+)\s*\(", header))
    from graphchainer_amd.api import EXPORTED_SYMBOLS
    assert declared == set(EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name) is not None


def test_no_cpu_fallback_without_gpu(lib):
    import graphchainer_amd as gca
    if gca.device_count() > 0:
        pytest.skip("a GPU is present")
    handle = C.c_void_p()
    rc = lib.gc_graph_create_from_gfa(os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa").encode(), C.byref(handle))
    assert rc == -3   # GC_ERR_DEVICE
    assert b"no CPU fallback" in lib.gc_last_error()


def test_product_does_not_touch_the_oracle():
    """The product sources must not include, link or import anything under oracle/."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "graphchainer_amd")):
        for f in files:
            if f.endswith((".so", ".pyc")):
                continue
            text = open(os.path.join(dirpath, f), errors="ignore").read()
            assert "oracle/" not in text.replace("under oracle/", "") and "from oracle" not in text and "import oracle" not in text, os.path.join(dirpath, f)


def test_every_environment_switch_of_the_product_is_documented():
    """the product library reads a fixed set of GC_* variables, and INTEGRATION.md §7 is the one table that lists them. The library reads them in
    one place, csrc/host/gc_switches.hpp: every name that header reads must appear in INTEGRATION.md, no other source may read one, and DESIGN.md stays one
    document with one numbering below 100 KB."""
    import re
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    header = os.path.join(csrc, "host", "gc_switches.hpp")
    names = set(re.findall(r'getenv\("(GC_[A-Z0-9_]+)"', open(header).read()))
    assert len(names) > 30
    for dirpath, dirs, files in os.walk(csrc):
        dirs[:] = [d for d in dirs if d != "build"]
        for f in files:
            path = os.path.join(dirpath, f)
            if path != header and f.endswith((".hip", ".hpp", ".cpp", ".h", ".inc")):
                text = open(path, errors="ignore").read()
                assert 'getenv("GC_' not in text and 'capacityOr("' not in text, path
    # r6 ("50 distinct getenv in the product"): what a HOST may set is at most 21 variables (25 before GC_ED_BLOCK / _HALF / _THIRD and GC_CHAIN_LARGE, which nothing
    # selected, went); everything a test uses to force a rare path or a small table is named GC_TEST_* (the switches of the measured-and-rejected alternatives went with their code)
    product = sorted(n for n in names if not n.startswith("GC_TEST_"))
    assert len(product) <= 21, product
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    shorthand = {"GC_TEST_EXT_MAX_PENDING": "GC_TEST_EXT_MAX_ITEMS / _PENDING / _TRACE", "GC_TEST_EXT_MAX_TRACE": "GC_TEST_EXT_MAX_ITEMS / _PENDING / _TRACE"}
    missing = sorted(n for n in names if n not in doc and shorthand.get(n, "\0") not in doc)
    assert not missing, f"not in INTEGRATION.md: {missing}"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert len(design.encode()) < 100_000
    heads = re.findall(r"^## (\d+)\. ", design, flags=re.M)
    assert heads == [str(i) for i in range(len(heads))], heads      # sections 0, 1, 2, ... once each, in order


def _build_shim_test(tmp_path):
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "shim_test")
    lib_dir = os.path.join(ROOT, "graphchainer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "shim", "shim_test.cpp"),
                           "-L" + lib_dir, "-lgraphchainer_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_shim_header_compiles_against_the_reference_type_names(tmp_path):
    """include/graphchainer_amd_shim.hpp (the reference's AlignOneWay / OrderSeeds / getSeeds / colinearChaining signatures over the C ABI)
    builds against minimal definitions of the reference's types and links with the library; without a GPU the program stops at graph
    creation (no CPU fallback)."""
    import subprocess
    import graphchainer_amd as gca
    exe = _build_shim_test(tmp_path)
    if gca.device_count() > 0:
        pytest.skip("a GPU is present: the gpu test runs the program")
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa"), "ACGTACGT"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "NO_DEVICE", out.stdout + out.stderr


def _build_multi_gpu_host(tmp_path):
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "multi_gpu_host")
    lib_dir = os.path.join(ROOT, "graphchainer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "multi_gpu_host.cpp"),
                           "-L" + lib_dir, "-lgraphchainer_amd", "-lpthread", "-Wl,-rpath," + lib_dir])
    return exe


def test_single_process_multi_gpu_host_builds_and_refuses_to_run_without_a_gpu(tmp_path):
    """examples/multi_gpu_host.cpp (one process, a worker thread per stream, a replica of the graph per device, one atomic batch cursor) builds against
    the C ABI alone; without a GPU it says so and stops (no CPU fallback). The GPU test runs it with two logical devices and compares with the oracle."""
    import subprocess
    import graphchainer_amd as gca
    exe = _build_multi_gpu_host(tmp_path)
    if gca.device_count() > 0:
        pytest.skip("a GPU is present: the gpu test runs the program")
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "syn20k.gfa"), os.path.join(ROOT, "tests", "golden", "syn20k.fa"), "2", "2", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "NO_DEVICE", out.stdout + out.stderr
