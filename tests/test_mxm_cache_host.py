"""The MUM / MEM index's cache file without a GPU: csrc/host/gc_mxm_cache.hpp (with the builder of csrc/host/gc_mxm_build.hpp) compiled with g++ into an ordinary program
(tests/mxm_cache_host/mxm_cache_host_test.cpp, with -fsanitize=address,undefined where the compiler has them, run directly): written, read back, damaged, truncated, of another
version, of another text; and through the library: gc_mxm_cache_check on a file that program wrote, and the order of gc_mxm_index_open's checks on a machine without a device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mxm_cache")
    out = str(tmp / "mxm_cache_host_test")
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    base = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "mxm_cache_host", "mxm_cache_host_test.cpp"), "-o", out]
    probe = str(tmp / "probe.cpp")
    open(probe, "w").write("int main() { return 0; }\n")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    has = subprocess.run(["g++"] + sanitize + [probe, "-o", str(tmp / "probe")], capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")], capture_output=True).returncode == 0
    subprocess.run(base + (sanitize if has else []), check=True, timeout=600)
    return out


@pytest.fixture(scope="module")
def lib():
    import graphchainer_amd as gca
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return gca.load_library()


def test_caches_round_trip_and_every_damaged_file_is_refused_untouched(exe, tmp_path):
    """40 random segments of 5 kb in all, an empty text, a one-letter segment, two identical segments: each cache reads back equal and no temporary file remains after a save.
    One flipped byte (magic, header, suffix array, checksum), four truncations, another version, a suffix-array entry beyond the text and a broken segment table under a
    valid checksum, and the fingerprint of a different text are refused with the file's name in the message, and the refused file's bytes are what they were. The predicate of the device
    build's limit is held at its boundary: 2^31 - 2 letters are taken, 2^31 - 1 are not."""
    work = tmp_path / "work"
    work.mkdir()
    out = subprocess.run([exe, "run", str(work)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
    assert sorted(p.suffix for p in work.iterdir()) == [".gcmxm"] * 5   # random, empty, one, twins, victim: nothing else was left


def test_the_library_checks_a_file_the_program_wrote(exe, lib, tmp_path):
    import graphchainer_amd as gca
    prefix = str(tmp_path / "random")
    out = subprocess.run([exe, "write", prefix], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    letters, segments, file_bytes, fingerprint = (int(x) for x in out.stdout.split())
    assert segments == 40 and 4500 < letters < 6500 and file_bytes == os.path.getsize(prefix + ".gcmxm")
    assert gca.api.mxm_cache_check(prefix) == {"version": 1, "text_letters": letters, "segments": segments, "file_bytes": file_bytes, "text_fingerprint": fingerprint}
    assert lib.gc_mxm_cache_check(prefix.encode(), None) == 0   # info may be NULL
    # refusals: GC_ERR_GRAPH (-2) with the file named, GC_ERR_INVALID (-1) without a prefix; the file stays as it is
    good = open(prefix + ".gcmxm", "rb").read()
    bad = bytearray(good)
    bad[len(bad) // 2] ^= 0x40
    open(prefix + ".gcmxm", "wb").write(bad)
    info = (C.c_uint64 * 5)()
    assert lib.gc_mxm_cache_check(prefix.encode(), info) == -2
    assert (prefix + ".gcmxm").encode() in lib.gc_last_error() and b"checksum" in lib.gc_last_error()
    assert open(prefix + ".gcmxm", "rb").read() == bytes(bad)
    with pytest.raises(RuntimeError, match="truncated"):
        open(prefix + ".gcmxm", "wb").write(good[:-9])
        gca.api.mxm_cache_check(prefix)
    assert lib.gc_mxm_cache_check(str(tmp_path / "nothing").encode(), info) == -2 and b"nothing.gcmxm" in lib.gc_last_error()
    assert lib.gc_mxm_cache_check(None, info) == -1 and lib.gc_mxm_cache_check(b"", info) == -1


def test_malformed_opens_are_refused_before_a_device_is_needed(lib):
    """gc_mxm_index_open checks its arguments on the host first: a null argument, a build mode of 2 and a non-zero `reserved` are GC_ERR_INVALID (-1) with or without a GPU (the
    graph handle is only read after these checks, so any non-null address stands in for one here)."""
    import graphchainer_amd as gca
    options = gca.api.GcMxmOptions(build=7, reserved=7, cache_prefix=b"x")
    lib.gc_mxm_options_default(C.byref(options))
    assert (options.build, options.reserved, options.cache_prefix) == (0, 0, None)
    lib.gc_mxm_options_default(None)
    handle = C.c_void_p(1)
    graph = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert lib.gc_mxm_index_open(None, C.byref(options), C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_mxm_index_open(graph, None, C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_mxm_index_open(graph, C.byref(options), None) == -1 and b"null" in lib.gc_last_error()
    options.build = 2
    assert lib.gc_mxm_index_open(graph, C.byref(options), C.byref(handle)) == -1 and b"neither GC_MXM_BUILD_HOST nor GC_MXM_BUILD_DEVICE" in lib.gc_last_error()
    assert not handle.value
    options.build, options.reserved = 1, 1
    assert lib.gc_mxm_index_open(graph, C.byref(options), C.byref(handle)) == -1 and b"reserved must be 0" in lib.gc_last_error()
    with pytest.raises(ValueError, match="'host' or 'device'"):
        gca.MxmIndex(None, build="gpu")
    assert {"gc_mxm_options_default", "gc_mxm_index_open", "gc_mxm_cache_check"} <= set(gca.api.EXPORTED_SYMBOLS)
