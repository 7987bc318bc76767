"""Low-complexity input without a device: the generator (tests/lowcomplexity.py) is deterministic, its tiers sit where they claim against the product's thresholds
(measured with the oracle alone, the thresholds read from the product's sources), and the independent Python models agree with the oracle on such input - the oracle
compiles the product's own minimizer and graph code, so on homopolymers and tandem arrays its word alone proves less than it seems."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lowcomplexity as lc                                        # noqa: E402
import test_alignment_model as alignment_check                    # noqa: E402
import test_seeding_model as seeding_check                        # noqa: E402
from graphchainer_amd.synth import SynthGraph                     # noqa: E402
from test_seeding_model import std_sort                           # noqa: E402,F401  (the fixture)

CSRC = os.path.join(ROOT, "graphchainer_amd", "csrc")


def product_thresholds():
    """The capacities the tiers are placed against, read from the sources that define them (never by running the product)."""
    kernels = open(os.path.join(CSRC, "hip", "gc_chain.hip")).read()
    long_policy = open(os.path.join(CSRC, "host", "gc_long_policy.hpp")).read()
    lds_anchors = int(re.search(r"#define CHAIN_LDS_ANCHORS (\d+)", kernels).group(1))
    assert "job.nSlots > 2 * LDS_ANCHORS" in kernels and "LDS == 2 ? CHAIN_LDS_ANCHORS / 2 : CHAIN_LDS_ANCHORS" in kernels
    first_cap = int(re.search(r"longFirstAlnCap\(uint64_t maxReadLen\) \{ return \(uint32_t\)std::max<uint64_t>\((\d+), maxReadLen / 512\); \}", long_policy).group(1))
    return {"small_class": lds_anchors // 2, "large_class": lds_anchors, "slot_routing_small": lds_anchors, "slot_routing_large": 2 * lds_anchors, "alignments": first_cap, "chain_16bit": 65535}


def per_read_counts(want, n):
    slots = want["frag_sr"] - want["frag_sl"]
    off = want["read_frag_off"]
    return {"seeds": np.diff(want["read_seed_off"]), "anchors": np.diff(want["read_anchor_off"]), "alignments": np.diff(want["read_longall_off"]),
            "slots": np.array([int(slots[off[r]:off[r + 1]].sum()) for r in range(n)], dtype=np.int64)}


def test_the_generator_is_deterministic_and_leaves_variant_sites_alone():
    a, reads_a, _ = lc.tier("c")
    b, reads_b, _ = lc.tier("c")
    assert np.array_equal(a.sg.backbone, b.sg.backbone) and a.blocks == b.blocks and reads_a == reads_b
    assert a.sg.gfa_lines() == b.sg.gfa_lines()
    plain = SynthGraph(60_000, seed=47, multi_allelic=0.1, nested=0.1)
    assert np.array_equal(plain.site_pos, a.sg.site_pos) and np.array_equal(plain.backbone[plain.site_pos], a.sg.backbone[a.sg.site_pos])
    inside = np.zeros(60_000, dtype=bool)
    for _, _, b0, b1 in a.blocks:
        inside[b0:b1] = True
    assert np.array_equal(plain.backbone[~inside], a.sg.backbone[~inside])           # nothing outside the returned spans was touched
    # the blocks are what they are called: a homopolymer is one letter away from its variant sites, an array repeats with its period
    g, _, _ = lc.tier("a")
    free = np.ones(60_000, dtype=bool)
    free[g.sg.site_pos] = False
    for kind, unit, b0, b1 in g.blocks:
        seq, ok = g.sg.backbone[b0:b1], free[b0:b1]
        same = (seq[unit:] == seq[:-unit]) & ok[unit:] & ok[:-unit]
        assert same.sum() == (ok[unit:] & ok[:-unit]).sum(), (kind, unit)
    kind, unit, b0, b1 = a.blocks[0]
    seq, ok = a.sg.backbone[b0:b1], free_mask(a)[b0:b1]
    both = ok[unit:] & ok[:-unit]
    differing = ((seq[unit:] != seq[:-unit]) & both).sum() / both.sum()
    assert kind == "diverged" and 0.02 < differing < 0.06, differing                   # two copies at 2 % each differ at ~4 % of their bases
    # reads of every placement, both strands
    assert len(g.inside(3, 4, 500, 1)) == 4 and len(g.crossing(0, 1600, 2)) == 3 and len(g.crossing(3, 1200, 2)) == 2 and 600 < len(g.spanning(0, 3)) < 2200
    assert g.read(7000, 300, 5, reverse=True) == g.read(7000, 300, 5, reverse=False).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def free_mask(g):
    free = np.ones(g.sg.backbone_len, dtype=bool)
    free[g.sg.site_pos] = False
    return free


TIER_RUNS = [("a", 35), ("a", 18), ("b", 35), ("b", 18), ("c", 35), ("c", 18), ("d", 35), ("d", 18), ("limit", 18)]


@pytest.mark.parametrize("name,split_gap", TIER_RUNS)
def test_tiers_sit_on_the_intended_side_of_the_thresholds(tmp_path, name, split_gap):
    """What makes each tier the tier it claims to be, from the oracle's counts per read: a generator that drifts fails here before the device tests turn ordinary."""
    from oracle import Oracle
    t = product_thresholds()
    assert t == {"small_class": 768, "large_class": 1536, "slot_routing_small": 1536, "slot_routing_large": 3072, "alignments": 32, "chain_16bit": 65535}
    g, reads, n_ordinary = lc.tier(name)
    gfa = str(tmp_path / "g.gfa")
    g.write_gfa(gfa)
    oracle = Oracle(gfa, long_pass=True, split_gap=split_gap)
    want = oracle.align(reads)
    c = per_read_counts(want, len(reads))
    print(name, split_gap, {k: v.tolist() for k, v in c.items()})
    assert not want["failed_assertion"].any()
    low = {k: v[:-n_ordinary] for k, v in c.items()}
    # the ordinary reads are ordinary: a chain, a handful of whole-read alignments, the small LDS class
    assert (c["anchors"][-n_ordinary:] > 20).all() and (c["anchors"][-n_ordinary:] < t["small_class"]).all() and (c["alignments"][-n_ordinary:] < 8).all()
    assert (np.diff(want["read_chain_off"])[-n_ordinary:] > 20).all()
    if name == "a":
        assert (low["seeds"] == 0).any() and ((low["seeds"] > 0) & (low["anchors"] == 0)).any() if split_gap == 35 else (low["seeds"] == 0).any()
        assert low["anchors"].max() < t["small_class"] and low["slots"].max() < t["slot_routing_small"] and low["seeds"].max() < 400
        assert low["alignments"].max() > t["alignments"]          # a read that crosses a homopolymer collects more alignments than the first capacity holds
    elif name == "b":
        assert low["alignments"].max() < t["alignments"]
        if split_gap == 35:   # reads on either side of both LDS classes and of both slot-routing limits
            assert (low["anchors"] < t["small_class"]).any() and ((low["anchors"] > t["small_class"]) & (low["anchors"] < t["large_class"])).any() and (low["anchors"] > t["large_class"]).any()
            assert (low["slots"] < t["slot_routing_small"]).any() and ((low["slots"] > t["slot_routing_small"]) & (low["slots"] < t["slot_routing_large"])).any() and (low["slots"] > t["slot_routing_large"]).any()
        else:
            assert (low["anchors"] > t["large_class"]).sum() >= 3 and low["anchors"].max() > 3500 and (low["slots"] > t["slot_routing_large"]).sum() >= 4
    elif name == "c":
        assert (low["alignments"] > t["alignments"]).sum() >= 2 and (low["alignments"] < t["alignments"]).sum() >= 2 and low["alignments"].min() >= 20
        assert low["anchors"].max() > (t["small_class"] if split_gap == 35 else t["large_class"])
    elif name == "d":
        assert low["seeds"].max() > 20_000 and low["alignments"].min() > 2 * t["alignments"]
        assert low["anchors"].min() > (6000 if split_gap == 35 else 12_000) and low["slots"].min() > 4 * t["slot_routing_large"]
    elif name == "limit":
        assert low["seeds"].max() > 20_000 and low["alignments"].max() > 4 * t["alignments"] and low["anchors"].max() > 12_000


def test_seeding_model_equals_the_oracle_on_low_complexity_reads(tmp_path, std_sort):   # noqa: F811
    """Reads in and across homopolymers, STRs and the exact unit-12 array (some of them without a single seed), then reads inside the unit-64 and unit-150 arrays
    (thousands of seeds with tied counts, goodness and positions), under the tie order libstdc++'s std::sort gives."""
    g, reads, _ = lc.tier("a")
    gfa = str(tmp_path / "a.gfa")
    g.write_gfa(gfa)
    from oracle import Oracle
    seeds = np.diff(Oracle(gfa, long_pass=False).align(reads)["read_seed_off"])
    assert (seeds == 0).sum() >= 2 and seeds.max() > 150
    compared, _ = seeding_check._check(gfa, reads, std_sort)
    assert compared == int(seeds.sum())
    g, reads, _ = lc.tier("c")
    gfa = str(tmp_path / "c.gfa")
    g.write_gfa(gfa)
    tandem = [reads[4][:1800], reads[5][:2000], reads[0][:1500], reads[3][-1500:]]
    compared, ties = seeding_check._check(gfa, tandem, std_sort)
    assert compared > 4000 and ties > 3000, (compared, ties)


def test_alignment_model_equals_the_oracle_on_a_tandem_read(tmp_path, std_sort):   # noqa: F811
    """The whole-read alignments (every trace cell) and the anchors of a 1.5 kb read inside the unit-150 array and of a 0.9 kb read inside the unit-64 array (14 alignments)."""
    g, reads, _ = lc.tier("c")
    gfa = str(tmp_path / "c.gfa")
    g.write_gfa(gfa)
    alignments, cells, anchors = alignment_check._check(gfa, [reads[5][:1500], reads[4][:900]], std_sort)
    assert alignments >= 15 and cells > 15_000 and anchors > 500, (alignments, cells, anchors)
