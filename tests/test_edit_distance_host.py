"""The unit step of the edit-distance kernels, the part that needs no GPU: csrc/hip/gc_editdist_core.hpp compiled with g++ (tests/ed_host/ed_core_test.cpp) and driven unit by
unit, as the lanes of a team of 21 and of 32, and over the whole matrix, with C = 1, 2, 4 and 8 columns per step, against a plain DP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ed_host") / "ed_core_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "ed_host", "ed_core_test.cpp"), "-o", out],
                   check=True, timeout=600)
    return out


def test_column_groups_give_the_distance_and_never_less(exe):
    """Lengths 1, C - 1, C, C + 1, 63-65, 127-129, 700, 64 TEAM - 1 .. 64 TEAM + 1 and 3 000 at error rates 0 to 0.5, m % C at 0, 1 and C - 1, both orders, 300 x 2 000 and its
    reverse, letters outside ACGT (a group that mixes both kinds included), k at 1, d / 2 + 1, d, d + 1, d + 8, 2 d + 3 and the cap: one banded pass never answers below the
    distance d and answers d whenever d <= k; every column a step reads is in the letter ring; a unit starts on a group its upper neighbour computes; at k equal to a team's
    limit (the shipped one and the formula's) a lane's consecutive units are disjoint in time, and one above it the lanes refuse with -2. Units of 2, 8 and 16 words run with
    their kernel's own columns per step (4, 1, 1) on one lane per unit and on three or two lanes at the formula's limit. Pairs whose optimal path follows the corridor's
    edge - X + S against S + Y and against S, |X| = |Y| = 1, 31, 64, 65, 300, S of 200 to 5 000 letters - at k = d - 1, d, d + 1, both orders, for every C."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
