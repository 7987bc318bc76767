"""Low-complexity test input (a test helper, not the product path): a SynthGraph with bubbles whose backbone carries homopolymer runs, short tandem repeats and
tandem arrays, and reads placed with respect to those blocks. Everything is a function of the arguments: fixed seeds, no global state.

The blocks overwrite backbone windows before the GFA is written. Bases at variant sites keep what SynthGraph drew (its alternative alleles were derived from them), so an
"exact" array is interrupted by a foreign base roughly every 50 bases - as a real array is by its SNPs.

TIERS names the inputs the low-complexity tests share (tests/test_low_complexity.py places them against the product's thresholds with the oracle alone,
tests/test_low_complexity_gpu.py runs them on the device)."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graphchainer_amd.synth import SynthGraph, _BASES, _COMP   # noqa: E402

KINDS = ("homopolymer", "str", "exact", "diverged")


def mutate(rng, s, rate):
    """The suite's read error model (tests/test_gpu_parity.py:_mutate): a third each of deletions, substitutions and insertions, `rng` a random.Random."""
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(rng.choice(b"ACGT"))
        else:
            out.append(ch)
        if rng.random() < rate / 3:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def block_sequence(rng, kind, unit, total, divergence=0.02):
    """`total` bases of one block. homopolymer: one letter; str / exact: a random unit of `unit` bases repeated; diverged: every copy of the unit carries its own
    substitutions at rate `divergence`."""
    if kind == "homopolymer":
        return np.full(total, _BASES[rng.integers(0, 4)], dtype=np.uint8)
    assert (kind == "str" and 2 <= unit <= 6) or kind in ("exact", "diverged"), (kind, unit)
    motif = _BASES[rng.integers(0, 4, size=unit)]
    while unit > 1 and len(set(motif.tolist())) == 1:      # (a unit of one letter would be a homopolymer)
        motif = _BASES[rng.integers(0, 4, size=unit)]
    seq = np.tile(motif, total // unit + 1)[:total].copy()
    if kind == "diverged":
        hit = rng.random(total) < divergence
        seq[hit] = _BASES[(np.searchsorted(_BASES, seq[hit]) + rng.integers(1, 4, size=int(hit.sum()))) % 4]
    return seq


class LowComplexityGraph:
    """SynthGraph(backbone_len, multi_allelic=0.1, nested=0.1) with `specs` = [(kind, unit, total), ...] written into its backbone in that order, `gap` random-backbone
    bases apart, the first block starting at `first`. .blocks = [(kind, unit, start, end)] in backbone coordinates."""

    def __init__(self, backbone_len, specs, seed=7, first=6000, gap=6000, divergence=0.02):
        self.sg = SynthGraph(backbone_len, seed=seed, multi_allelic=0.1, nested=0.1)
        rng = np.random.default_rng(seed + 5000011)
        free = np.ones(backbone_len, dtype=bool)
        free[self.sg.site_pos] = False                     # variant sites keep their bases
        self.blocks = []
        at = first
        for kind, unit, total in specs:
            assert kind in KINDS and at + total + gap <= backbone_len, (kind, at, total, backbone_len)
            seq = block_sequence(rng, kind, unit, total, divergence)
            window = slice(at, at + total)
            self.sg.backbone[window] = np.where(free[window], seq, self.sg.backbone[window])
            self.blocks.append((kind, unit, at, at + total))
            at += total + gap
        self.end_of_blocks = at - gap

    def write_gfa(self, path):
        return self.sg.write_gfa(path)

    def read(self, start, length, seed, reverse=None):
        """A haplotype walk from backbone coordinate `start`, 5-8 % errors, `length` letters; the strand is drawn unless given."""
        rng = random.Random(seed)
        hap = self.sg.haplotype_window(np.random.default_rng(seed), int(start), int(length * 1.12) + 48).tobytes()
        seq = mutate(rng, hap, rng.uniform(0.05, 0.08))[:length]
        if rng.random() < 0.5 if reverse is None else reverse:
            seq = _COMP[np.frombuffer(seq, dtype=np.uint8)[::-1]].tobytes()
        return seq

    def inside(self, block, n, length, seed):
        """n reads that lie wholly inside blocks[block], alternating strands."""
        _, _, b0, b1 = self.blocks[block]
        room = (b1 - b0) - int(length * 1.12) - 48
        assert room > 0, (self.blocks[block], length)
        rng = random.Random(seed)
        return [self.read(b0 + rng.randrange(room), length, seed + 17 * i, reverse=bool(i & 1)) for i in range(n)]

    def crossing(self, block, length, seed):
        """Reads that enter and leave blocks[block]: one over its left edge, one over its right edge, one that starts before it and ends behind it when `length` allows."""
        _, _, b0, b1 = self.blocks[block]
        out = [self.read(max(0, b0 - length // 2), length, seed, reverse=False), self.read(b1 - length // 2, length, seed + 1, reverse=True)]
        if length > (b1 - b0) + 200:
            out.append(self.read(max(0, b0 - (length - (b1 - b0)) // 2), length, seed + 2))
        return out

    def spanning(self, block, seed, flank=150):
        """One read from inside blocks[block] across the random backbone between them to inside blocks[block + 1]."""
        (_, _, a0, a1), (_, _, c0, c1) = self.blocks[block], self.blocks[block + 1]
        start = max(a0, a1 - flank)
        return self.read(start, min(c1, c0 + flank) - start, seed)

    def ordinary(self, n, length, seed):
        """n reads from the random backbone behind the last block."""
        lo, hi = self.end_of_blocks + 500, self.sg.backbone_len - int(length * 1.12) - 600
        assert hi > lo, (lo, hi)
        rng = random.Random(seed)
        return [self.read(rng.randrange(lo, hi), length, seed + 29 * i) for i in range(n)]


def tier(name):
    """(LowComplexityGraph, reads, number of ordinary reads at the end of `reads`) of a named tier."""
    if name == "a":       # homopolymers, STRs, an exact unit-12 array: few or no seeds; reads inside, over the edges, through, and from block to block
        g = LowComplexityGraph(60_000, [("homopolymer", 1, 300), ("homopolymer", 1, 1000), ("str", 2, 400), ("str", 3, 1500), ("str", 6, 900), ("exact", 12, 1200)], seed=41, first=3000, gap=1500)
        reads = g.inside(1, 2, 600, 3) + g.inside(3, 2, 800, 5) + g.inside(4, 2, 500, 6) + g.inside(5, 2, 800, 7)
        for b in range(6):
            reads += g.crossing(b, 1600 if b in (0, 2) else 2700, 100 + 10 * b)
        reads += [g.spanning(b, 200 + b, flank=f) for b, f in ((0, 150), (2, 200), (4, 400))]
    elif name == "b":     # unit 2000 / unit 500 arrays of 12 kb, 10 kb reads: 650-4 660 anchors per read, across both LDS classes of k_chain and its slot routing
        g = LowComplexityGraph(80_000, [("diverged", 2000, 12_000), ("diverged", 500, 12_000)], seed=43, first=5000, gap=7000)
        reads = g.inside(0, 2, 10_000, 11) + g.inside(1, 2, 10_000, 13) + g.crossing(0, 10_000, 15)[:1] + g.crossing(1, 10_000, 17)[1:2]
    elif name == "c":     # unit 64 x 3 kb and unit 150 x 4 kb, reads a little longer than the arrays: 22-40 whole-read alignments per read
        g = LowComplexityGraph(60_000, [("diverged", 64, 3000), ("diverged", 150, 4000)], seed=47, first=5000, gap=6000)
        reads = [g.read(5000 - 600, 4200, 21, reverse=False), g.read(5000 - 600, 4200, 22, reverse=True), g.read(14_000 - 600, 5200, 23, reverse=False), g.read(14_000 - 600, 5200, 24, reverse=True)]
        reads += g.inside(0, 1, 2400, 25) + g.inside(1, 1, 3200, 26)
    elif name == "d":     # unit 150 x 12 kb, 10 kb reads: 25 k seeds, 7.5 k / 14 k anchors, ~78 whole-read alignments per read
        g = LowComplexityGraph(70_000, [("diverged", 150, 12_000)], seed=53, first=6000, gap=6000)
        reads = g.inside(0, 2, 10_000, 31)
    elif name == "limit":   # one 10 kb read in a unit-64 array of 12 kb: the read nearest k_chain's 16-bit limits that the oracle aligns in seconds
        g = LowComplexityGraph(70_000, [("diverged", 64, 12_000)], seed=59, first=6000, gap=6000)
        reads = g.inside(0, 1, 10_000, 37)
    else:
        raise KeyError(name)
    n_ordinary = 3
    return g, reads + g.ordinary(n_ordinary, 3000, 71), n_ordinary


TIERS = ("a", "b", "c", "d")
