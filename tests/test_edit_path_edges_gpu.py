"""k_edit_path (gca.api.edit_path, csrc/hip/gc_edpath.hip) on the fixed points of its code, tests/edit_path_cases.py: nearly identical strings above edlib's 1 MB limit
(distance 0-5: where the oracle once gave no alignment), the largest directly traced problem and the smallest split one at 1, 2, 6 and 65 blocks, leaves of two and three
strips of 64 blocks (the store indexed [block][column], the walk back across strips), sweeps of 1 023 .. 4 097 columns under two strips (the letter and carry rings of 4 096
slots, refilled 2 048 ahead every 1 024 steps, the carries flushed 63 columns behind), 8 193 rows against 63 and 64 columns more, IUPAC codes and lower case. All pairs in
one call; equality is op for op with the oracle (oracle/edlib_path.hpp), with the real edlib's recorded output (tests/golden/ref_units.expected.npz, "edit_path_edges")
and with the real edlib itself where oracle/_ref is built. tests/test_gpu_parity.py::test_edit_path_kernel holds the random sizes."""
import numpy as np
import pytest

from edit_path_cases import assert_is_alignment, edit_path_cases, gpu_subset, is_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


def test_edit_path_on_the_kernels_fixed_points(gca):
    from oracle import RefUnits
    from oracle.binding import oracle_edit_path
    from test_oracle_units import REF_GOLDEN, edit_path_record
    cases = edit_path_cases()
    recorded = np.load(REF_GOLDEN)["edit_path_edges"]
    assert len(recorded) == len(cases)
    chosen = gpu_subset(cases)
    blocks = {}
    for i in chosen:
        blocks[cases[i][0].split("/")[0]] = blocks.get(cases[i][0].split("/")[0], 0) + 1
    assert blocks == {"near": 48, "limit": 8, "strips": 3, "rings": 14, "letters": 4}
    assert sum(is_split(cases[i][1], cases[i][2]) for i in chosen) >= 70
    dist, ops = gca.api.edit_path([cases[i][1] for i in chosen], [cases[i][2] for i in chosen])
    try:
        ref = RefUnits()
    except (FileNotFoundError, OSError):
        ref = None
    wrong = []
    for i, d, o in zip(chosen, dist, ops):
        name, q, t = cases[i]
        d = int(d)
        want_d, want_ops = oracle_edit_path(q, t)
        ok = len(o) > 0 and d == want_d and np.array_equal(o, want_ops) and np.array_equal(edit_path_record(d, o), recorded[i])
        if ok and ref is not None:
            ref_d, ref_ops = ref.edit_path(q, t)
            ok = d == ref_d and np.array_equal(o, ref_ops)
        if not ok:
            rec_d, rec_len = (int(x) for x in recorded[i][:16].view(np.int64))
            wrong.append((name, len(q), len(t), d, want_d, rec_d, len(o), len(want_ops), rec_len))
            continue
        assert_is_alignment(q, t, d, o, name)
    assert not wrong, f"{len(wrong)} of {len(chosen)} (name, Q, T, distance: device / oracle / edlib, ops: device / oracle / edlib): {wrong[:12]}"
