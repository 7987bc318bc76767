"""tests/precise_model.py (--precise-clipping, --X-drop) on the CPU: it is BandModel / GlobalModel with clipping off; what clipping does to clean and to junk-tailed
reads; every rule of the mode on the graph and reads the GPU tests use; the two forms of the column maximum against each other; the (cells, score) pairs at which a
fused multiply-subtract would give another X score; and the C ABI's extension block: its defaults and the combinations it refuses, with no device present."""
import ctypes
import os
import random
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import test_extension_model as tem   # noqa: E402
from band_model import BandModel   # noqa: E402
from extension_model import W, ModelAssertion   # noqa: E402
from global_model import GlobalModel   # noqa: E402
from precise_model import PreciseModel, error_cost, max_x_score_cells, max_x_score_words, x_score   # noqa: E402
from test_band_model import _noisy_cases, load_from, run, tangle   # noqa: E402
from test_global_alignment_gpu import Inputs, model_results   # noqa: E402
from test_seeding_model import std_sort   # noqa: E402,F401

FIELDS = ("slice_min", "slice_nodes", "slice_min_cell", "failed", "score", "trace")
CUTOFFS = (0.5, 0.66, 0.7, 0.9)
X_DROPS = (0, 5, 50)
CLIP_RULES = ("clip: best slice is not the last", "clip: ends before the read's end", "xdrop: stop", "xdrop: first slice dropped")


def _graph(tmp_path, where):
    if where == "golden":
        return load_from(tem.GOLD, "syn20k.gfa", 10)[1]
    return load_from(tangle(tmp_path, 5), "tangle.gfa", 10)[1]


@pytest.mark.parametrize("where", ["golden", "tangle"])
def test_with_clipping_off_it_is_the_band_and_the_global_model(tmp_path, where):
    """The inputs of tests/test_global_model.py, result for result; with the ramp too."""
    g = _graph(tmp_path, where)
    for band in ({}, {"ramp_bandwidth": 14}):
        pairs = [(BandModel(g, 10, **band), PreciseModel(g, 10, **band)), (GlobalModel(g, 10, **band), PreciseModel(g, 10, force_global=True, **band))]
        compared = 0
        for big, offset, text in _noisy_cases(g, random.Random(31), 25, 700):
            for old, new in pairs:
                want, got = run(old, big, offset, text), run(new, big, offset, text)
                assert (want is None) == (got is None)
                if want is not None:
                    assert all(want[k] == got[k] for k in FIELDS)
                    compared += 1
        assert compared >= 30
        for old, new in pairs:
            assert old.fired == new.fired


def _linear_case(g, rng, length):
    """A walk through the graph from a random cell: (bigraph id, offset, the `length` letters that follow that cell - an extension's row 0 is the letter after the seed's)."""
    while True:
        node = rng.randrange(len(g.length))
        inside = rng.randrange(g.length[node])
        text = tem.walk_from(g, rng, node, inside, length + 1)
        if len(text) == length + 1:
            return g.node_ids[node], g.node_offset[node] + inside, text[1:]


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_a_clean_read_is_aligned_to_its_last_base(cutoff):
    g = _graph(None, "golden")
    rng = random.Random(5)
    for length in (50, 64, 128, 300):
        big, offset, text = _linear_case(g, rng, length)
        for x_drop in X_DROPS:
            got = PreciseModel(g, 10, precise_clipping=cutoff, x_drop=x_drop).extend(text, big, offset)
            assert not got["failed"] and got["score"] == 0
            assert got["trace"][0][2] == length - 1 and got["trace"][-1][2] == -1


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_a_junk_tail_is_clipped_near_the_junction(cutoff):
    """backbone + random letters. The alignment ends at the cell with the best X score = cells - score * E. At the junction the score is 0 and X = junction; a cell d rows
    past it with s edits has X = junction + d - s * E. So the end is never before the junction, and it lies d rows past it only if those d random letters align with
    fewer than (d + 1) / E edits (truncation gives less than one).
    The bound on d. Through a band of 10 over a graph with a variant every ~45 bases a random letter finds a free match less than half the time: a stretch of d junk
    rows costs at least d / 2 - 1 edits (the - 1: a lucky first letter or two). With the inequality above, d / 2 - 1 < (d + 1) / E, i.e. d < 2 (E + 1) / (E - 2) for E > 2:
    8 rows at c = 0.66 (E = 2.94), 6 at 0.7, 2 at 0.9. At c = 0.5, E = 2: every edit pays for two rows, which is what random letters cost - no bound from this argument but
    the slice, d <= W, since a row 64 past the junction needs 32 junk edits to stay level and the walk is biased down. Asserted per cut-off as derived; the measured d is printed."""
    g = _graph(None, "golden")
    rng = random.Random(11)
    E = error_cost(cutoff)
    bound = W if E <= 2 else int(2 * (E + 1) / (E - 2))
    for length in (100, 170, 260):
        big, offset, text = _linear_case(g, rng, length)
        read = text + "".join(rng.choice("ACGT") for _ in range(200))
        got = PreciseModel(g, 10, precise_clipping=cutoff).extend(read, big, offset)
        assert not got["failed"]
        end = got["trace"][0][2] + 1
        d = end - length
        print("cutoff", cutoff, "E", E, "junction", length, "end", end, "d", d, "bound", bound, "score", got["score"])
        assert 0 <= d <= bound
        assert got["score"] < (d + 1) / E


def _fused_pairs(cutoff, max_score=3000):
    """The (cells <= 64, score < max_score) at which cells - score * E rounded ONCE (a fused multiply-subtract) truncates to another integer than the product and
    the difference rounded each: exact rationals of the double E."""
    E = error_cost(cutoff)
    exact = Fraction(E)
    out = set()
    for cells in range(1, W + 1):
        for score in range(max_score):
            fused = cells - score * exact
            if int(float(fused)) != x_score(cells, score, E):
                out.add((cells, score))
    return out


def test_where_a_fused_multiply_subtract_would_differ():
    assert (51, 17) in _fused_pairs(0.66, 100)
    E = error_cost(0.66)
    assert E == 2.9411764705882355 and x_score(51, 17, E) == 1 and int(float(51 - 17 * Fraction(E))) == 0
    assert len(_fused_pairs(0.7)) == 1609
    for cutoff in (0.5, 0.75, 0.9):
        assert not _fused_pairs(cutoff)


def _column_rows(vp, vn, score_end):
    """The 64 row values of a column from its words."""
    rows, value = [0] * W, score_end
    for r in range(W - 1, -1, -1):
        rows[r] = value
        value -= ((vp >> r) & 1) - ((vn >> r) & 1)
    return rows, value   # (the rows, the score before the first)


# a read for the fused pair of 0.66: 17 edits in its first rows, then clean - row 50 of the first slice holds (51 cells, score 17) when nothing else is cheaper.
# (Added here: whether Inputs' own reads reach a pair is a property of those inputs, which the test below reports.)
def _extra_reads(inputs):
    bb = inputs.bb
    head = bytearray(bb[33000:33100])
    for i in range(1, 35, 2):
        head[i] = ord("A") if head[i] != ord("A") else ord("C")
    return [bytes(bb[32900:33000]) + bytes(head) + bytes(bb[33100:33300])]


@pytest.fixture(scope="module")
def clipped_runs(tmp_path_factory, std_sort):   # noqa: F811
    """Every cut-off x X-drop on Inputs' whole reads (whole-read pass and 35-base fragments) and its 64-base fragment reads: the rules fired and the columns seen."""
    inputs = Inputs(tmp_path_factory.mktemp("precise"))
    fired, columns = {}, {}
    for cutoff in CUTOFFS:
        seen = set()
        for x_drop in X_DROPS:
            for reads, whole, split in ((inputs.whole + _extra_reads(inputs), True, 35), (inputs.fragments, False, 64)):
                _, ext = model_results(inputs.gfa, reads, std_sort, PreciseModel, 10, whole, split, split, precise_clipping=cutoff, x_drop=x_drop)
                for rule, n in ext.fired.items():
                    fired[rule] = fired.get(rule, 0) + n
                seen.update(ext.columns_seen)
        columns[cutoff] = seen
    return fired, columns


def test_every_rule_fires_on_the_gpu_tests_inputs(clipped_runs):
    fired, _ = clipped_runs
    print({rule: n for rule, n in fired.items() if rule.startswith(("clip:", "xdrop:"))})
    for rule in CLIP_RULES:
        assert fired.get(rule, 0) > 0, rule
    assert "trim: slice dropped" not in fired


def test_the_two_forms_of_the_column_maximum_agree(clipped_runs):
    """maxXScoreLocalMinima (what the reference runs) against maxXScoreCellByCell (what it asserts under EXTRACORRECTNESSASSERTIONS) over all 64 rows - the form
    calculateNodeInner uses - on every distinct column the runs looked at."""
    _, columns = clipped_runs
    compared = 0
    for cutoff, seen in columns.items():
        E = error_cost(cutoff)
        for vp, vn, score_end in seen:
            rows, before = _column_rows(vp, vn, score_end)
            assert max_x_score_words(vp, vn, before, E) == max_x_score_cells(np.array([before] + rows), E), (cutoff, vp, vn, score_end)
            compared += 1
    print("columns compared:", compared)
    assert compared > 20_000


@pytest.mark.parametrize("cutoff", [0.66, 0.7])
def test_the_inputs_reach_a_pair_where_fusing_would_differ(clipped_runs, cutoff):
    _, columns = clipped_runs
    pairs = _fused_pairs(cutoff, 400)
    hit = set()
    for vp, vn, score_end in columns[cutoff]:
        rows, _ = _column_rows(vp, vn, score_end)
        hit.update((r + 1, rows[r]) for r in range(W) if (r + 1, rows[r]) in pairs)
    print("cutoff", cutoff, "pairs reached:", sorted(hit)[:10], "of", len(pairs))
    assert hit


# ---- the C ABI's extension block

def _lib():
    from graphchainer_amd.api import load_library
    return load_library()


def test_gc_params_ext_default():
    from graphchainer_amd.api import GcParamsExt
    e = GcParamsExt()
    e.struct_size, e.x_drop, e.precise_clipping = 1, 77, 0.5
    _lib().gc_params_ext_default(ctypes.byref(e))
    assert (e.struct_size, e.x_drop, e.precise_clipping) == (ctypes.sizeof(GcParamsExt), 0, 0.0)
    assert ctypes.sizeof(GcParamsExt) == 16 and GcParamsExt.precise_clipping.offset == 8


@pytest.mark.parametrize("seeded", [False, True])
def test_invalid_extension_blocks_are_refused_without_a_device(seeded):
    """Every check of the block happens before the handles are looked at: the calls below hand over pointers to zeroed memory for them (never read), and come back
    with GC_ERR_INVALID and the field's name whether or not a device is present."""
    from graphchainer_amd.api import GcParams, GcParamsExt, GcResult
    lib = _lib()
    dummy = [ctypes.create_string_buffer(4096) for _ in range(4)]
    g, s, st, reads = (ctypes.cast(d, ctypes.c_void_p) for d in dummy)

    def call(force_global=0, **fields):
        p, e = GcParams(), GcParamsExt()
        lib.gc_params_default(ctypes.byref(p))
        lib.gc_params_ext_default(ctypes.byref(e))
        p.force_global = force_global
        for k, v in fields.items():
            setattr(e, k, v)
        res = ctypes.POINTER(GcResult)()
        rc = lib.gc_align_batch_ext(g, None if seeded else s, st, reads, s if seeded else None, ctypes.byref(p), ctypes.byref(e), ctypes.byref(res))
        return rc, lib.gc_last_error().decode()

    cases = [
        (dict(struct_size=ctypes.sizeof(GcParamsExt) + 8), "struct_size"),
        (dict(x_drop=-1), "x_drop"),
        (dict(precise_clipping=0.0005), "precise_clipping"),
        (dict(precise_clipping=0.9995), "precise_clipping"),
        (dict(precise_clipping=1.0), "precise_clipping"),
        (dict(precise_clipping=-0.5), "precise_clipping"),
        (dict(precise_clipping=float("nan")), "precise_clipping"),
        (dict(precise_clipping=float("inf")), "precise_clipping"),
        (dict(x_drop=5, force_global=1), "force_global"),
        (dict(x_drop=5, precise_clipping=0.66, force_global=1), "force_global"),
    ]
    for fields, said in cases:
        rc, message = call(**fields)
        assert rc == -1 and said in message, (fields, rc, message)
    # both a seeder and seeds, or neither: refused too (with a valid block)
    p, e = GcParams(), GcParamsExt()
    lib.gc_params_default(ctypes.byref(p))
    lib.gc_params_ext_default(ctypes.byref(e))
    res = ctypes.POINTER(GcResult)()
    for a, b in ((s, s), (None, None)):
        assert lib.gc_align_batch_ext(g, a, st, reads, b, ctypes.byref(p), ctypes.byref(e), ctypes.byref(res)) == -1
        assert b"not both" in lib.gc_last_error()
