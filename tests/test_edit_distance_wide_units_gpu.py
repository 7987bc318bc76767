"""k_edit_distance<G> for the units of 2, 4, 8 and 16 words (csrc/hip/gc_editdist.hip), which run 4, 2, 1 and 1 columns per step (edColsOfUnit) and, from 8 words on, one
wave per SIMD: gca.edit_distance against the oracle's distance on pairs sent straight to each of them. launchEditDistances gives a pair with first band K and a read (second
argument) of n bases the unit G when K >= 4 000 G / 2, n > 4 096 G / 2 and 2 K < n; GC_ED_FIRST_K sets K. Per unit, at the largest read with one unit per lane (64 units) and
at one where lane 0 takes a second unit (65):
  (a) X + S against S + Y, |X| = |Y| = (K - 20) / 2: the optimal path follows both edges of the corridor, so a corridor one diagonal too narrow changes the answer;
  (b) S against X + S, |X| = K - 20: the overhang, one edge;
  (c) a 3 % mutation with the path's length at 0 and at C - 1 modulo the unit's columns per step;
  (d) (a) with |X| = |Y| = K / 2 + 10: the distance is above K, the first pass fails and the band grows (64 units), or the lanes cannot hold twice the band and the pair
      moves on (65 units): to the next unit's turn and the workgroup kernel for the units below 16, to a last pass at the widest band the lanes hold for the unit of 16.
Both orders where the swapped pair's read still routes to the same unit. The line GC_DEBUG_TIMES prints tells which kernels a call launched: every pair of a call is in its
unit's class and none in the workgroup kernel's. tests/test_edit_distance_host.py drives the same core with the same units on the host."""
import random
import re
import time

import pytest

from test_edit_distance_columns_gpu import _mutate, gca, oracle_distance  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# G: (GC_ED_FIRST_K, read length with 64 units, with 65 units)
ROWS = {2: (4000, 8100, 8300), 4: (8000, 16200, 16500), 8: (16000, 32400, 33000), 16: (32000, 64800, 65700)}
COLS_OF_UNIT = {2: 4, 4: 2, 8: 1, 16: 1}                                      # edColsOfUnit at GC_ED_COLS = 8
CLASS_OF_UNIT = {2: 3, 4: 4, 8: 5, 16: 6}                                     # position in "3 per wave, 2 per wave, units 1..16, workgroup per pair"
CLASSES = re.compile(r"edit distance classes \([^)]*\):((?: \d+){8})")


def _seq(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def _routes_to_unit(G, K, n):
    return K >= 4000 * G // 2 and K < 4000 * G and n > 4096 * G // 2 and 2 * K < n


def _pairs(G):
    """[(kind, path, read)] of one row."""
    K, n64, n65 = ROWS[G]
    C = COLS_OF_UNIT[G]
    rng = random.Random(1000 + G)
    out = []
    for n in (n64, n65):
        assert (n + 64 * G - 1) // (64 * G) == (64 if n == n64 else 65)
        for kind, h in (("a", (K - 20) // 2), ("d", K // 2 + 10)):
            S = _seq(rng, n - h)
            out.append((kind, _seq(rng, h) + S, S + _seq(rng, h)))
        S = _seq(rng, n - (K - 20))
        out.append(("b", S, _seq(rng, K - 20) + S))
        for rem in sorted({0, C - 1}):
            read = _seq(rng, n)
            path = _mutate(rng, read, 0.03)
            while len(path) % C != rem:
                path += _seq(rng, 1)
            out.append(("c", path, read))
    return out


def _launch(gca, capfd, G, paths, reads):
    """The distances of one call and the class counts it printed."""
    print(capfd.readouterr().out, end="")                                     # (stderr starts empty; what the test has printed so far stays in its report)
    began = time.perf_counter()
    got = list(map(int, gca.edit_distance(paths, reads)))
    seconds = time.perf_counter() - began
    captured = capfd.readouterr()
    print(captured.out, end="")
    err = captured.err
    lines = CLASSES.findall(err)
    assert len(lines) == 1, err
    counts = [int(x) for x in lines[0].split()]
    print(f"unit {G}: {len(paths)} pairs, classes {counts}, {seconds:.3f} s")
    return got, counts


@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_wide_unit(gca, oracle_distance, monkeypatch, capfd, G):   # noqa: F811
    K = ROWS[G][0]
    pairs = _pairs(G)
    want = [oracle_distance(path, read) for _, path, read in pairs]
    for (kind, path, read), d in zip(pairs, want):                           # conditions on the input, not on the kernel
        assert _routes_to_unit(G, K, len(read)), (kind, len(read))
        if kind in "ab":
            assert K - 40 <= d <= K, (kind, len(read), d)
        if kind == "d":
            assert d > K, (kind, len(read), d)
        if kind == "c":
            assert d < K // 4, (kind, len(read), d)
    monkeypatch.setenv("GC_ED_FIRST_K", str(K))
    monkeypatch.setenv("GC_DEBUG_TIMES", "1")
    got, counts = _launch(gca, capfd, G, [p for _, p, _ in pairs], [r for _, _, r in pairs])
    assert counts[CLASS_OF_UNIT[G]] == len(pairs) and counts[7] == 0 and sum(counts) == len(pairs), counts
    assert got == want, [(kind, len(read), g, w) for (kind, _, read), g, w in zip(pairs, got, want) if g != w]
    swapped = [(kind, read, path, d) for (kind, path, read), d in zip(pairs, want) if _routes_to_unit(G, K, len(path))]
    assert {kind for kind, _, _, _ in swapped} == {"a", "c", "d"}              # (the overhang's shorter string is no read for this unit)
    got, counts = _launch(gca, capfd, G, [p for _, p, _, _ in swapped], [r for _, _, r, _ in swapped])
    assert counts[CLASS_OF_UNIT[G]] == len(swapped) and counts[7] == 0 and sum(counts) == len(swapped), counts
    assert got == [d for _, _, _, d in swapped], [(kind, len(read), g, d) for (kind, _, read, d), g in zip(swapped, got) if g != d]
