"""The whole-read kernel's node-record accessors (hip/gc_device.hpp) on the host: tests/node_rec_host/node_rec_host_test.cpp compiles them with g++, as
tests/frag_host compiles the fragment core, and checks every accessor against the graph arrays for every node of twelve random CSR graphs of 2 000..3 500
nodes - lengths 1 and 64, in- and out-degrees 0, 1, 254, 255, 256 and 300 (the record's 8-bit degree fields saturate at 255), ambiguous nodes, and node n - 1
in each of these roles. Built twice: as it is, and as its own executable with the address and undefined-behaviour sanitizers, under which a read behind
the end of an array (a record n, outOff[n + 1], ambSeq words of a plain node) ends the run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "node_rec_host", "node_rec_host_test.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_node_record_accessors_equal_the_graph_arrays(tmp_path, flags):
    exe = tmp_path / "node_rec_host_test"
    subprocess.run(["g++", "-std=c++17", "-w", "-I/opt/rocm/include"] + flags + [SRC, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "NODE_REC_HOST_OK" in out.stdout, out.stdout + out.stderr
    fields = out.stdout.split()
    assert int(fields[fields.index("nodes") + 1]) > 24_000 and int(fields[fields.index("ambiguous") + 1]) > 100
