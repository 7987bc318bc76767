"""The band controls (--ramp-bandwidth, --tangle-effort) of tests/band_model.py against the oracle where the oracle can judge them, and the rules
themselves on inputs built to make them apply. Plus the C ABI's defaults for the two gc_params fields."""
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


def load_from(directory, gfa, bandwidth):
    gold, tem.GOLD = tem.GOLD, str(directory)
    try:
        return tem.load(gfa, bandwidth)
    finally:
        tem.GOLD = gold


def tangle(tmp_path, seed=7, segments=160):
    (tmp_path / "tangle.gfa").write_text(tem.tangle_gfa(random.Random(seed), segments))
    return tmp_path


def run(model, big, offset, text):
    try:
        return model.extend(text, big, offset)
    except ModelAssertion:
        return None


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(a[k] == b[k] for k in ("slice_min", "slice_nodes", "slice_min_cell", "failed", "score", "trace"))


@pytest.mark.parametrize("where,gfa,bandwidth,count,max_len,seed", [
    ("golden", "syn20k.gfa", 10, 30, 900, 21),
    ("golden", "ref_test_graph.gfa", 10, 20, 300, 22),
    ("tangle", "tangle.gfa", 3, 40, 400, 23),
])
def test_band_model_with_both_off_equals_the_oracle(tmp_path, where, gfa, bandwidth, count, max_len, seed):
    o, g = load_from(tem.GOLD if where == "golden" else tangle(tmp_path), gfa, bandwidth)
    model = BandModel(g, bandwidth)
    compared = 0
    for big, offset, text in tem.cases(g, random.Random(seed), count, max_len):
        compared += tem.compare(o, model, big, offset, text) is not None
    assert compared >= count // 2
    assert not any(rule.startswith(("ramp:", "cells:")) for rule in model.fired)


@pytest.mark.parametrize("ramp", [12, 20, 35])
def test_one_slice_with_the_ramp_is_the_wider_band(tmp_path, ramp):
    """Slice 0 always runs with the ramp bandwidth and a rewind needs an earlier slice: an extension of at most 64 rows (every fragment extension)
    at -b 10 -B ramp is the oracle's extension at -b ramp, the slice's stored bandwidth (which the backtrace reads) included."""
    o, g = load_from(tangle(tmp_path), "tangle.gfa", ramp)
    model = BandModel(g, 10, ramp_bandwidth=ramp)
    rng = random.Random(ramp)
    compared = 0
    for big, offset, text in tem.cases(g, rng, 80, 60):
        text = text[:W - 1]
        compared += tem.compare(o, model, big, offset, text) is not None
    assert compared >= 40
    assert "ramp: rewind" not in model.fired


def _noisy_cases(g, rng, count, length):
    for _ in range(count):
        node = rng.randrange(len(g.length))
        inside = rng.randrange(g.length[node])
        text = tem.mutate(rng, tem.walk_from(g, rng, node, inside, length), 0.2)
        if rng.random() < 0.5 and len(text) > 200:                # leaves the graph half-way
            cut = rng.randrange(100, len(text) - 50)
            text = text[:cut] + "".join(rng.choice("ACGT") for _ in range(len(text) - cut))
        yield g.node_ids[node], g.node_offset[node] + inside, text


def _table_is_consistent(model, big, offset, text):
    table = model.slices(text, big, offset)
    for a, b in zip(table, table[1:]):
        assert b.j == a.j + W
        assert b.min_score >= a.min_score
    return table


def test_the_ramp_rewinds_and_keeps_the_table_consistent(tmp_path):
    o, g = load_from(tangle(tmp_path, 5), "tangle.gfa", 10)
    model = BandModel(g, 4, ramp_bandwidth=12)
    plain = BandModel(g, 4)
    differ = 0
    for big, offset, text in _noisy_cases(g, random.Random(31), 25, 700):
        got = run(model, big, offset, text)
        differ += not same(got, run(plain, big, offset, text))
        try:
            _table_is_consistent(model, big, offset, text)
        except ModelAssertion:
            pass
    assert model.fired.get("ramp: rewind", 0) > 0
    assert differ > 0


def test_the_cell_limit_breaks_and_flags_the_slice(tmp_path):
    o, g = load_from(tangle(tmp_path, 9), "tangle.gfa", 10)
    unlimited = BandModel(g, 10)
    cases = list(_noisy_cases(g, random.Random(41), 20, 500))
    for big, offset, text in cases:
        run(unlimited, big, offset, text)
    cells = sorted(unlimited.slice_cells)
    limit = cells[len(cells) // 4]                                    # a quarter of the slices reach it
    model = BandModel(g, 10, max_cells_per_slice=limit)
    for big, offset, text in cases:
        got = run(model, big, offset, text)
        if got is not None:
            try:
                _table_is_consistent(model, big, offset, text)
            except ModelAssertion:
                pass
    assert model.fired.get("cells: break", 0) > 0
    assert model.fired.get("cells: scores not valid", 0) > 0


def test_a_limit_above_every_slice_changes_nothing(tmp_path):
    o, g = load_from(tangle(tmp_path, 9), "tangle.gfa", 10)
    unlimited = BandModel(g, 10)
    cases = list(_noisy_cases(g, random.Random(43), 15, 500))
    want = [run(unlimited, *c) for c in cases]
    limited = BandModel(g, 10, max_cells_per_slice=max(unlimited.slice_cells) + 1)
    assert all(same(run(limited, *c), w) for c, w in zip(cases, want))
    assert not any(rule.startswith("cells:") for rule in limited.fired)


def test_gc_params_default_turns_the_band_controls_off():
    """gc_params gained ramp_bandwidth and max_cells_per_slice after `capacity`: the defaults are the reference's (0: no ramp, -1: unlimited)."""
    from graphchainer_amd.api import GcParams, load_library
    lib = load_library()
    p = GcParams()
    p.ramp_bandwidth, p.max_cells_per_slice = 77, 77
    lib.gc_params_default(ctypes.byref(p))
    assert p.ramp_bandwidth == 0
    assert p.max_cells_per_slice == -1
    assert p.bandwidth == 10
    assert GcParams.ramp_bandwidth.offset == GcParams.capacity.offset + GcParams.capacity.size
