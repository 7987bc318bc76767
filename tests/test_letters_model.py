"""tests/letters_inputs.py on the CPU: the rewritten graph and the reads put the extension modes' models on IUPAC nodes and letters often enough to mean something
(counted on the models' own results, and printed), and with every mode off the models are the oracle on these inputs. tests/test_letters_gpu.py holds the device
to the same models; an anchor whose path holds an ambiguous node cannot come from the lockstep fragment kernel, which declines such nodes, so the floors
on such anchors here are what shows that the slab kernels ran on them there."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from band_model import BandModel                                         # noqa: E402
from global_model import GlobalModel                                     # noqa: E402
from letters_inputs import CODES, SETS, LettersInputs                   # noqa: E402
from precise_model import PreciseModel                                   # noqa: E402
from test_alignment_model import _check                                  # noqa: E402
from test_precise_model import CLIP_RULES                                # noqa: E402
from test_seeding_model import std_sort                                  # noqa: E402,F401

MODES = [("band default", BandModel, {}), ("force_global", GlobalModel, {}), ("clipping at 0.66", PreciseModel, {"precise_clipping": 0.66})]
CLIP_SETTINGS = [(0.66, 0), (0.66, 5), (0.7, 0)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return LettersInputs(tmp_path_factory.mktemp("letters"))


def coverage(inputs, std_sort):   # noqa: F811
    """Per mode: (trace cells, on ambiguous nodes, letters under them, anchors of the 35-base run, ambiguous ones, anchors of the 64-base run, ambiguous ones)."""
    out = {}
    for name, cls, kw in MODES:
        whole, _ = inputs.run(std_sort, cls, "whole", True, **kw)
        frags, _ = inputs.run(std_sort, cls, "fragments", False, split=64, **kw)
        out[name] = inputs.trace_letters(whole) + inputs.anchor_paths(whole) + inputs.anchor_paths(frags)
    return out


def test_the_inputs_hold_the_cases(inputs, std_sort):   # noqa: F811
    amb = inputs.ambiguous()
    print("ambiguous split nodes:", sum(amb), "of", len(amb), "codes placed:", len(inputs.placed),
          "holding their base:", sum(base in SETS[code] for base, code in inputs.placed.values()))
    assert sum(amb) >= 200
    assert len(inputs.whole) + len(inputs.fragments) <= 30 and max(len(r) for r in inputs.whole + inputs.fragments) <= 1000
    for name, (cells, on_amb, letters, a35, a35_amb, a64, a64_amb) in coverage(inputs, std_sort).items():
        print(f"{name}: trace cells {cells}, on ambiguous nodes {on_amb}; 35-base anchors {a35}, with an ambiguous node {a35_amb}; 64-base anchors {a64}, with one {a64_amb}; letters {letters}")
        assert on_amb >= 0.10 * cells > 0
        assert a35_amb >= 0.15 * a35 > 0
        assert a64_amb >= 0.15 * a64 > 0
        if name == "band default":
            assert set(letters) == set(CODES)                                  # every code lies under a trace cell
    band, _ = inputs.run(std_sort, BandModel, "whole", True)
    reverse = [r for r in inputs.iupac_reads if any(trace[0][0] & 1 for _, _, _, trace in band[r][0])]
    print("IUPAC reads aligned on the reverse strand:", reverse, "alignments per read:", [len(b[0]) for b in band])
    assert reverse
    for r in inputs.no_seed_reads:                                             # U for T: no seed, so nothing - and no assertion
        assert inputs.seeds(std_sort, inputs.whole[r]) == [] and band[r] == ([], [])
    for r in inputs.hand_built:
        if r not in inputs.no_seed_reads:
            assert band[r] is not None and band[r][0], f"read {r} is not aligned"
    assert all(b is not None for b in band)


def test_the_modes_rules_fire(inputs, std_sort):   # noqa: F811
    """What the modes' own GPU tests require of their inputs, on these."""
    fired = {}
    for cutoff, x_drop in CLIP_SETTINGS:
        _, ext = inputs.run(std_sort, PreciseModel, "whole", True, precise_clipping=cutoff, x_drop=x_drop)
        assert ext.fired.get("clip: ends before the read's end", 0) > 0 and ext.fired.get("clip: best slice is not the last", 0) > 0
        if x_drop:
            assert ext.fired.get("xdrop: stop", 0) > 0
        for rule, n in ext.fired.items():
            fired[rule] = fired.get(rule, 0) + n
    # (tests/test_precise_model.py sums the rules over its cut-offs up to 0.9: a first slice is dropped only where one edit costs more than the X-drop, E = 10 > 5)
    for which, whole, split, cutoff, x_drop in [("fragments", False, 64) + CLIP_SETTINGS[0], ("fragments", False, 64) + CLIP_SETTINGS[1], ("whole", True, 35, 0.9, 5)]:
        _, ext = inputs.run(std_sort, PreciseModel, which, whole, split=split, precise_clipping=cutoff, x_drop=x_drop)
        for rule, n in ext.fired.items():
            fired[rule] = fired.get(rule, 0) + n
    print({rule: n for rule, n in fired.items() if rule.startswith(("clip:", "xdrop:"))})
    for rule in CLIP_RULES:
        assert fired.get(rule, 0) > 0, rule
    _, unlimited = inputs.run(std_sort, BandModel, "whole", True)
    cells = sorted(unlimited.slice_cells)
    limit = cells[len(cells) // 4]
    _, ext = inputs.run(std_sort, BandModel, "whole", True, max_cells_per_slice=limit)
    print("cell limit", limit, {k: v for k, v in ext.fired.items() if k.startswith("cells:")})
    assert any(c >= limit for c in ext.slice_cells) and ext.fired.get("cells: break", 0) > 0
    _, ext = inputs.run(std_sort, BandModel, "whole", True, ramp_bandwidth=25)
    print("ramp", {k: v for k, v in ext.fired.items() if k.startswith("ramp:")})
    assert ext.fired.get("ramp: rewind", 0) > 0
    _, ext = inputs.run(std_sort, GlobalModel, "whole", True)
    assert any(rule.startswith("global:") for rule in ext.fired)


def _oracle_per_read(want, n):
    out = []
    for r in range(n):
        alns = []
        for a in range(int(want["read_longall_off"][r]), int(want["read_longall_off"][r + 1])):
            t0, t1 = int(want["long_trace_off"][a]), int(want["long_trace_off"][a + 1])
            trace = list(zip(want["long_trace_node"][t0:t1].tolist(), want["long_trace_offset"][t0:t1].tolist(), want["long_trace_seqpos"][t0:t1].tolist(),
                             [bool(x) for x in want["long_trace_switch"][t0:t1]]))
            alns.append((int(want["longall_start"][a]), int(want["longall_end"][a]), int(want["longall_score"][a]), trace))
        anchors = []
        for b in range(int(want["read_anchor_off"][r]), int(want["read_anchor_off"][r + 1])):
            anchors.append((int(want["anchor_x"][b]), int(want["anchor_y"][b]), int(want["anchor_score"][b]),
                            want["anchor_path"][int(want["anchor_path_off"][b]):int(want["anchor_path_off"][b + 1])].tolist()))
        out.append((alns, anchors))
    return out


def test_with_every_mode_off_the_models_equal_the_oracle(inputs, std_sort):   # noqa: F811
    """The base model with the anchors' end cells (tests/test_alignment_model.py's check), then BandModel and PreciseModel at their defaults: whole-read alignments with
    every trace cell and the anchors with their paths, read by read; and PreciseModel with clipping off is BandModel / GlobalModel result for result."""
    from oracle import Oracle
    alignments, cells, anchors = _check(inputs.gfa, inputs.whole, std_sort)
    print("base model against the oracle: alignments", alignments, "trace cells", cells, "anchors", anchors)
    assert alignments >= len(inputs.whole) - 2 and anchors > 100
    want = Oracle(inputs.gfa, long_pass=True).align(inputs.whole)
    assert not any(want["failed_assertion"])
    per_read = _oracle_per_read(want, len(inputs.whole))
    band, band_ext = inputs.run(std_sort, BandModel, "whole", True)
    off, off_ext = inputs.run(std_sort, PreciseModel, "whole", True)
    assert band == per_read
    assert off == band and off_ext.fired == band_ext.fired
    glob, glob_ext = inputs.run(std_sort, GlobalModel, "whole", True)
    forced, forced_ext = inputs.run(std_sort, PreciseModel, "whole", True, force_global=True)
    assert forced == glob and forced_ext.fired == glob_ext.fired
    want = Oracle(inputs.gfa, long_pass=False, split_len=64, split_gap=64).align(inputs.fragments)
    frags, _ = inputs.run(std_sort, BandModel, "fragments", False, split=64)
    assert [f[1] for f in frags] == [p[1] for p in _oracle_per_read(want, len(inputs.fragments))]
    assert frags == inputs.run(std_sort, PreciseModel, "fragments", False, split=64)[0]


def test_without_the_codes_the_coverage_is_gone(tmp_path, std_sort):   # noqa: F811
    """The same inputs with the IUPAC codes left out of the graph: no ambiguous node, so the floors above cannot be met by ACGT input."""
    plain = LettersInputs(tmp_path, iupac=False)
    assert sum(plain.ambiguous()) == 0
    whole, _ = plain.run(std_sort, BandModel, "whole", True)
    cells, on_amb, letters = plain.trace_letters(whole)
    assert cells > 0 and on_amb == 0 and not letters
    assert plain.anchor_paths(whole)[1] == 0
