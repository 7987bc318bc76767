"""The forced global alignment (--global-alignment) of tests/global_model.py against tests/band_model.py: what the default keeps is a prefix of what
the forced run keeps, the two agree where the default drops nothing, and the ramp reaches slice 0 only. Plus the C ABI's default for
gc_params::force_global."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import test_extension_model as tem   # noqa: E402
from band_model import BandModel   # noqa: E402
from extension_model import ModelAssertion, W   # noqa: E402
from global_model import GlobalModel   # noqa: E402
from test_band_model import _noisy_cases, load_from, run, tangle   # noqa: E402

FIELDS = ("slice_min", "slice_nodes", "slice_min_cell", "failed", "score", "trace")


def _graph(tmp_path, where):
    if where == "golden":
        return load_from(tem.GOLD, "syn20k.gfa", 10)[1]
    return load_from(tangle(tmp_path, 5), "tangle.gfa", 10)[1]


def _dropped(model):
    return sum(n for rule, n in model.fired.items() if rule.startswith(("stop:", "trim:")))


@pytest.mark.parametrize("where", ["golden", "tangle"])
def test_the_default_table_is_a_prefix_of_the_forced_one(tmp_path, where):
    g = _graph(tmp_path, where)
    plain, forced = BandModel(g, 10), GlobalModel(g, 10)
    for big, offset, text in _noisy_cases(g, random.Random(31), 25, 700):
        want = forced.extend(text, big, offset)                    # (no ModelAssertion: the forced run never fails)
        assert len(want["slice_min"]) == (len(text) + W - 1) // W + 1
        assert not want["failed"]
        got = run(plain, big, offset, text)
        if got is None:
            continue
        n = len(got["slice_min"])
        for key in ("slice_min", "slice_nodes", "slice_min_cell"):
            assert got[key] == want[key][:n], key
    assert _dropped(plain) > 0
    assert any(rule.startswith("global:") for rule in forced.fired)
    assert not any(rule.startswith(("stop:", "trim:", "ramp:")) for rule in forced.fired)


@pytest.mark.parametrize("where", ["golden", "tangle"])
def test_where_nothing_is_dropped_nothing_changes(tmp_path, where):
    g = _graph(tmp_path, where)
    plain, forced = BandModel(g, 10), GlobalModel(g, 10)
    rng = random.Random(37)
    compared = 0
    for k in range(20):
        node = rng.randrange(len(g.length))
        inside = rng.randrange(g.length[node])
        text = tem.mutate(rng, tem.walk_from(g, rng, node, inside, 400), (0.0, 0.02, 0.05)[k % 3])
        if not text:
            continue
        big, offset = g.node_ids[node], g.node_offset[node] + inside
        before = _dropped(plain)
        got = run(plain, big, offset, text)
        if got is None or _dropped(plain) != before:
            continue
        want = forced.extend(text, big, offset)
        for key in FIELDS:
            assert got[key] == want[key], key
        compared += 1
    assert compared >= 10


def test_the_ramp_reaches_slice_0_only(tmp_path):
    g = _graph(tmp_path, "tangle")
    forced = GlobalModel(g, 4, ramp_bandwidth=12)
    tables = 0
    for big, offset, text in _noisy_cases(g, random.Random(31), 25, 700):
        try:
            table = forced.slices(text, big, offset)
        except ModelAssertion:
            continue
        assert len(table) == (len(text) + W - 1) // W + 1
        assert table[1].bandwidth == 12
        assert all(s.bandwidth == 4 for s in table[2:])
        tables += len(table) > 2
    assert tables >= 15
    assert "ramp: rewind" not in forced.fired


def test_gc_params_default_turns_the_forced_global_alignment_off():
    """gc_params gained force_global directly behind max_cells_per_slice; the default is the reference's (off), the other defaults are as they were."""
    from graphchainer_amd.api import GcParams, load_library
    lib = load_library()
    p = GcParams()
    p.force_global, p.ramp_bandwidth, p.max_cells_per_slice = 77, 77, 77
    lib.gc_params_default(ctypes.byref(p))
    assert p.force_global == 0
    assert GcParams.force_global.offset == GcParams.max_cells_per_slice.offset + GcParams.max_cells_per_slice.size
    assert p.ramp_bandwidth == 0
    assert p.max_cells_per_slice == -1
    assert (p.bandwidth, p.split_len, p.split_gap, p.colinear_gap, p.seed_density) == (10, 35, 35, 10000, 10.0)
    assert (p.long_pass, p.keep_traces, p.keep_seeds, p.stitch, p.edit_distances, p.device_output, p.e_cutoff) == (0, 0, 0, 1, 1, 0, -1.0)
