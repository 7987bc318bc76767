"""The MUM / MEM seeder without a GPU: the suffix-array builder of csrc/host/gc_mxm_build.hpp and the per-position routine of csrc/hip/gc_mxm_core.hpp compiled with g++ into an
ordinary program (tests/mxm_host/mxm_host_test.cpp, with -fsanitize=address,undefined where the compiler has them), held to a naive suffix sort and to tests/mxm_model.py;
and the order of gc_seeds_mxm's checks on a machine without a device."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mxm_model as mm                         # noqa: E402
from test_mxm_model import HAND_CASES          # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mxm")
    out = str(tmp / "mxm_host_test")
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    base = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(csrc, "hip"), os.path.join(ROOT, "tests", "mxm_host", "mxm_host_test.cpp"), "-o", out]
    probe = str(tmp / "probe.cpp")
    open(probe, "w").write("int main() { return 0; }\n")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    has = subprocess.run(["g++"] + sanitize + [probe, "-o", str(tmp / "probe")], capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")], capture_output=True).returncode == 0
    subprocess.run(base + (sanitize if has else []), check=True, timeout=600)
    return out


def test_suffix_arrays_equal_a_naive_sort_and_the_homopolymer_is_not_quadratic(exe):
    """A random 5 kb text of 40 segments, a 1000-letter homopolymer, a 600-letter AC repeat, IUPAC letters, one-letter and empty-after-mapping segments, no segment at all: the
    builder's suffix array is the naive sort's, the packed text gives every letter back, and the homopolymer builds in well under a second (sanitizers included)."""
    out = subprocess.run([exe, "sa"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def _run_case(exe, tmp_path, segments, reads, mode, min_len, count, prefix_len):
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(f"{mode} {min_len} {-1 if count is None else count} {prefix_len}\nS {len(segments)}\n")
        for i in sorted(segments):
            f.write(f"{i} {segments[i] or '*'}\n")
        f.write(f"R {len(reads)}\n")
        for r in reads:
            f.write((r or "*") + "\n")
    out = subprocess.run([exe, "hits", path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    got, lines = [], out.stdout.split("\n")
    at = 0
    for r in range(len(reads)):
        tag, index, n = lines[at].split()
        assert tag == "R" and int(index) == r
        got.append([tuple(int(x) for x in l.split()) for l in lines[at + 1:at + 1 + int(n)]])
        at += 1 + int(n)
    return got


@pytest.mark.parametrize("prefix_len", [0, 2, 4])
def test_hand_cases_on_one_lane(exe, tmp_path, prefix_len):
    """Every hand-checked case through the core header, as ordered lists, with and without a prefix table (min_len below, at and above its letters)."""
    for name, segments, read, mode, min_len, count, want in HAND_CASES:
        assert _run_case(exe, tmp_path, segments, [read], mode, min_len, count, prefix_len) == [want], name


@pytest.mark.parametrize("mode", [mm.MEM, mm.MUM])
def test_random_and_repetitive_texts_against_the_model(exe, tmp_path, mode):
    """Segments with repeats, homopolymers, IUPAC letters and an empty one; reads cut from them on both strands with errors, N and a read shorter than min_len; min_len across
    the table boundary (table of 5 letters: 3 below, 5 at, 9 above, 40 beyond one word), count all and cutting through ties."""
    rng = random.Random(1234 + mode)
    rep = "".join(rng.choice("ACGT") for _ in range(60))
    segments = {}
    for i in range(1, 25):
        s = "".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 200)))
        if i % 4 == 0:
            s = s[:30] + rep[:rng.randrange(20, 60)] + s[30:]
        if i % 5 == 0:
            s = s[:10] + "A" * rng.randrange(5, 80) + s[10:]
        if i % 6 == 0:
            s = s[:15] + rng.choice("NRYW") + s[15:]
        segments[i] = s
    segments[30], segments[31] = "", "NN"
    comp = str.maketrans("ACGTNRYW", "TGCANYRW")
    reads = ["", "A", "ACGTNACGT"]
    for k in range(12):
        s = segments[rng.randrange(1, 25)]
        a = rng.randrange(0, max(1, len(s) - 20))
        r = list(s[a:a + rng.randrange(10, 150)])
        for _ in range(len(r) // 25):
            r[rng.randrange(len(r))] = rng.choice("ACGTN")
        r = "".join(r)
        reads.append(r.translate(comp)[::-1] if k & 1 else r)
    reads.append("A" * 70)
    text = mm.Text(segments)
    for min_len, count in ((3, None), (5, None), (9, None), (9, 3), (40, None), (5, 7)):
        want = [mm.seeds(text, r.encode(), mode, min_len, count) for r in reads]
        assert sum(len(w) for w in want) > (0 if min_len == 40 and mode == mm.MUM else 2)
        assert _run_case(exe, tmp_path, segments, reads, mode, min_len, count, 5) == want, (min_len, count)


def test_malformed_calls_are_refused_before_a_device_is_needed():
    """gc_seeds_mxm, gc_mxm_index_create and gc_seeds_hits check their arguments on the host first: a null handle is GC_ERR_INVALID (-1) with or without a GPU."""
    import graphchainer_amd as gca
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = gca.load_library()
    handle = C.c_void_p()
    assert lib.gc_mxm_index_create(None, C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_seeds_mxm(None, None, None, 2, 1, 20, C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    n = C.c_uint64()
    assert lib.gc_seeds_hits(None, C.byref(handle), C.byref(handle), C.byref(n)) == -1
    assert not handle.value
    lib.gc_mxm_index_destroy(None)
    assert {"gc_mxm_index_create", "gc_mxm_index_destroy", "gc_mxm_index_array", "gc_seeds_mxm", "gc_seeds_hits"} <= set(gca.api.EXPORTED_SYMBOLS)
