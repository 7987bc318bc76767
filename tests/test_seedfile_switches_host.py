"""GC_TEST_SEEDFILE_PIECE and GC_TEST_SEEDFILE_HASH_BITS, the seed store's two test hooks, as csrc/host/gc_switches.hpp reads them (tests/seedfile_host/
seedfile_switches_test.cpp prints the two fields): defaults, ordinary values, one value below, at and above each bound; both are in INTEGRATION.md §7's table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("-", 32 << 20, 64)]
CASES += [(f"GC_TEST_SEEDFILE_PIECE={v}", want, 64) for v, want in ((-1, 1), (0, 1), (1, 1), (2, 2), (4096, 4096), (1 << 33, 1 << 33))]          # max(1, atoll)
CASES += [(f"GC_TEST_SEEDFILE_HASH_BITS={v}", 32 << 20, want) for v, want in ((0, 1), (1, 1), (2, 2), (20, 20), (63, 63), (64, 64), (65, 64))]   # 1..64
CASES += [("GC_TEST_SEEDFILE_PIECE=300 GC_TEST_SEEDFILE_HASH_BITS=2", 300, 2)]


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_seed_store_switches_are_parsed(tmp_path, sanitize):
    exe = str(tmp_path / "seedfile_switches_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "seedfile_host", "seedfile_switches_test.cpp"), "-o", exe], check=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GC_")}
    run = subprocess.run([exe], input="".join(c[0] + "\n" for c in CASES), capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")[:-1]
    assert got == [f"testSeedfilePiece={piece} testSeedfileHashBits={bits}" for _, piece, bits in CASES]


def test_the_seed_store_switches_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "graphchainer_amd", "csrc", "host", "gc_switches.hpp")).read()
    for name in ("GC_TEST_SEEDFILE_PIECE", "GC_TEST_SEEDFILE_HASH_BITS"):
        assert name in doc and f'seedfileSwitch("{name}")' in header
