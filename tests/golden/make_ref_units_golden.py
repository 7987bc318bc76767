"""Records the reference units' outputs (oracle/_ref/libref_units.so: the reference's WordSlice.h, AlignmentCorrectnessEstimation.cpp and
edlib, compiled by `make -C oracle ref` where the reference tree lies) for the seeded inputs of tests/test_oracle_units.py and of
tests/test_gpu_parity.py::test_edit_path_kernel, into ref_units.expected.npz (run here, result committed). The tests compare with the
live units where they are built and with this recording elsewhere.

Keys: one per entry of test_oracle_units.RECORDED - "edit_path_edges" among them, the pairs of tests/edit_path_cases.py, which tests/test_edit_path_edges_gpu.py reads too -
and "gpu_edit_path". A path case is 32 bytes: distance, op count, digest of the ops. Every key already in the file must come out as it is there, unless --replace names it.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

from oracle import RefUnits  # noqa: E402
from test_gpu_parity import _path_pairs  # noqa: E402
from test_oracle_units import RECORDED, REF_GOLDEN, edit_path_record  # noqa: E402


def main():
    ref = RefUnits()
    out = {name: fn(ref) for name, fn in RECORDED.items()}
    out["gpu_edit_path"] = np.array([edit_path_record(*ref.edit_path(a, b)) for a, b in _path_pairs(random.Random(99))])
    replace = sys.argv[sys.argv.index("--replace") + 1:] if "--replace" in sys.argv else []
    if os.path.exists(REF_GOLDEN):
        with np.load(REF_GOLDEN) as old:
            for name in old.files:
                if name not in replace and not (name in out and np.array_equal(old[name], out[name])):
                    sys.exit(f"{name}: the reference units no longer give what {os.path.basename(REF_GOLDEN)} holds (nothing written)")
    np.savez_compressed(REF_GOLDEN, **out)
    for name, a in out.items():
        print(name, a.shape, a.dtype)


if __name__ == "__main__":
    main()
