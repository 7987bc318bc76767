"""The whole-read kernel's column loop (hip/gc_column_asm.hpp: unrolled twice, an odd-column tail, three segments of the node's code stream)
against the oracle on a graph whose nodes take every length 1..64, each on the backbone and inside a bubble: odd and even lengths for the tail,
1 and 2 for an empty and a one-column loop, 32 / 33 / 34 and 63 / 64 for the changes of code word. The reads carry ONT-like errors and span dozens
of slices, so a node is met new in a slice, carried with nothing to repair and carried with a repaired first row. Each setting of the column
store is held to the oracle: the default (the DP leaves its columns in the lanes and the backtrace loads them), none (the DP writes two lane
words per column and the backtrace runs the loop again), and a store too small for most extensions (the long reads outgrow it and are rerun in the plain layout, the short ones fit)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, _mutate, _revcomp, compare, gca, run_case   # noqa: E402,F401

READ_LEN = 3000
SHORT_READ_LEN = 250
ERROR_RATE = 0.10


def every_length_graph(seed=5):
    """(GFA text, one haplotype). Per length L in 1..64 (shuffled): a backbone segment of L bases, a bubble with two arms of L bases, a 64-base
    spacer. No segment is longer than a split node, so a segment is a node of its own length. The backbone segment of length L starts with base
    L % 4 and its arms with the two after it; segments longer than 32 carry base (L + 1) % 4 .. at column 32, the start of the second code word."""
    import random
    rng = random.Random(seed)
    rand = lambda n: bytearray(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    segs, links, hap = [], [], bytearray()

    def seg(seq):
        segs.append(bytes(seq))
        return len(segs)

    lengths = list(range(1, 65))
    rng.shuffle(lengths)
    prev = [seg(rand(64))]
    hap += segs[0]
    for L in lengths:
        trio = []
        for k in range(3):   # backbone, arm, arm
            s = rand(L)
            s[0] = b"ACGT"[(L + k) % 4]
            if L > 32:
                s[32] = b"ACGT"[(L + k + 1) % 4]
            trio.append(s)
        if trio[2] == trio[1]:
            trio[2][-1] = b"ACGT"[(b"ACGT".index(trio[1][-1]) + 1) % 4]
        b = seg(trio[0])
        links += [(p, b) for p in prev]
        x, y = seg(trio[1]), seg(trio[2])
        links += [(b, x), (b, y)]
        sp = seg(rand(64))
        links += [(x, sp), (y, sp)]
        hap += trio[0] + trio[1 + rng.randrange(2)] + segs[sp - 1]
        prev = [sp]
    text = "".join("S\t%d\t%s\n" % (i + 1, s.decode()) for i, s in enumerate(segs)) + "".join("L\t%d\t+\t%d\t+\t0M\n" % l for l in links)
    return text, bytes(hap), segs


def reads_over(hap, seed=23):
    import random
    rng = random.Random(seed)
    reads = []
    step = (len(hap) - READ_LEN) // 5
    for i in range(6):
        r = _mutate(rng, hap[i * step:i * step + READ_LEN], ERROR_RATE)
        reads.append(_revcomp(r) if i % 2 else r)
    for start in (1000, 5000):   # two reads of a few slices, whose columns fit the small store
        reads.append(_mutate(rng, hap[start:start + SHORT_READ_LEN], ERROR_RATE))
    return reads


def test_graph_has_every_node_length_and_every_base_at_both_code_words():
    text, hap, segs = every_length_graph()
    assert set(b"".join(segs)) <= set(b"ACGT")   # no IUPAC symbol: every node takes the lean column loop
    by_length = {}
    for s in segs:
        by_length.setdefault(len(s), []).append(s)
    assert sorted(by_length) == list(range(1, 65)) and all(len(v) >= 3 for v in by_length.values())
    for column in (0, 1, 32, 33):
        for parity in (0, 1):   # odd and even node lengths
            seen = {s[column] for s in segs if len(s) > column + 1 and len(s) % 2 == parity}
            assert seen == set(b"ACGT"), (column, parity)
    assert len(hap) > 2 * READ_LEN


@pytest.mark.gpu
@pytest.mark.parametrize("capacities", [None, {"long_column_store": -1}, {"long_column_store": 700}], ids=["store", "no-store", "small-store"])
def test_every_node_length_against_the_oracle(gca, tmp_path, capacities):
    text, hap, segs = every_length_graph()
    gfa = str(tmp_path / "lengths.gfa")
    open(gfa, "w").write(text)
    reads = reads_over(hap)
    got, want = run_case(gca, gfa, reads, long_pass=True, capacities=capacities)
    node_lengths = set(int(x) for x in gca.AlignmentGraph(gfa).array("nodeLength"))
    assert node_lengths >= set(range(1, 65))
    # not vacuous: every read has a whole-read alignment in the oracle, and none of them left the one-extension-per-wave kernel
    assert np.all(np.diff(np.asarray(want["read_longall_off"])) >= 1), np.diff(np.asarray(want["read_longall_off"]))
    fallback, column_steps = int(got["counters_long"][7]), int(got["counters_long"][2])
    print(f"capacities {capacities}: plain-layout reruns {fallback} of {len(reads)} reads, column steps {column_steps}")
    if capacities == {"long_column_store": 700}:
        # what outgrows the store answers an overflow and its read is rerun in the plain layout - that is the setting (the long reads all do);
        # the short reads fit it and stay in the one-extension-per-wave kernel, with a store that is nearly full
        assert 0 < fallback <= len(reads) - 2, fallback
    else:
        assert fallback == 0, "a read went to the plain-layout fallback"
    assert column_steps > 0
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
