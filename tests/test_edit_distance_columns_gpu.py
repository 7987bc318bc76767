"""The edit-distance kernels step through the matrix a group of C columns at a time (csrc/hip/gc_editdist_core.hpp): gca.edit_distance against the oracle's plain DP, both
orders, at the smallest shapes where the groups can go wrong - one past each letter ring, the lengths from which a lane takes a second unit, either side of the bands at which
a pair changes kernel, the workgroup kernel with a ragged last group, and matrices smaller than a group or a word. tests/test_edit_distance_host.py drives the same core
on the host; this file is about the kernels around it (rings in LDS, the shuffle between lanes, the hand-over through LDS, the rerun path). It stays with the team kernels,
k_edit_distance<1> and the workgroup kernel; the units of 2 to 16 words are launched by tests/test_edit_distance_wide_units_gpu.py."""
import ctypes as C
import os
import random
import re

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CORE = open(os.path.join(ROOT, "graphchainer_amd", "csrc", "hip", "gc_editdist_core.hpp")).read()
COLS = int(re.search(r"#define GC_ED_COLS (\d+)", _CORE).group(1))               # columns per step
HALF_KMAX = int(re.search(r"ED_HALF_KMAX = (\d+),", _CORE).group(1))              # first band (exclusive) of two pairs per wave
THIRD_KMAX = (64 + COLS) * (21 - 1) + 2                                           # and of three: one past the widest band 21 lanes of 64 rows hold, (rows + C)(lanes - 1) + 1


def _mutate(rng, s, rate):
    out = bytearray()
    for ch in s:
        if rng.random() < rate:
            what = rng.randrange(3)
            if what == 0:
                out.append(rng.choice(b"ACGT"))
            elif what == 1:
                out.append(ch)
                out.append(rng.choice(b"ACGT"))
        else:
            out.append(ch)
    return bytes(out)


def _seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _columns(rng, path, rem):
    """The path with letters added until its length is rem modulo COLS."""
    while len(path) % COLS != rem % COLS:
        path += bytes([rng.choice(b"ACGT")])
    return path


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


@pytest.fixture(scope="module")
def oracle_distance():
    from oracle import Oracle  # noqa: F401  (builds the oracle library)
    from oracle.binding import load_oracle_lib
    lib = load_oracle_lib()
    lib.gco_edit_distance.restype = C.c_uint64
    lib.gco_edit_distance.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    known = {}

    def distance(a, b):
        if (a, b) not in known:
            known[(a, b)] = known[(b, a)] = len(a) + len(b) if not a or not b else int(lib.gco_edit_distance(a, len(a), b, len(b)))
        return known[(a, b)]
    return distance


def _check(gca, oracle_distance, pairs, note=""):
    """gca.edit_distance(paths, reads): the first of a pair gives the columns, the second the rows - both orders."""
    want = [oracle_distance(a, b) for a, b in pairs]
    assert list(map(int, gca.edit_distance([p[0] for p in pairs], [p[1] for p in pairs]))) == want, note
    assert list(map(int, gca.edit_distance([p[1] for p in pairs], [p[0] for p in pairs]))) == want, note + " (reversed)"


@pytest.fixture(scope="module")
def ring_pairs():
    rng = random.Random(41)
    pairs = []
    for length in (2049, 4097, 8193):                                            # one past each ring: three, two and one pair per wave
        for rem in (0, 1, COLS - 1):
            path = _columns(rng, _seq(rng, length), rem)
            pairs.append((path, _mutate(rng, path, 0.02)))
    return pairs


@pytest.mark.parametrize("first_k", [None, "200", "2000"])
def test_ring_refills(gca, oracle_distance, ring_pairs, monkeypatch, first_k):
    """Paths one letter longer than each ring, m % C at 0, 1 and C - 1, at 2 % error: the default first band (two pairs per wave), a small bound (three per wave) and one
    beyond both teams (one pair per wave; the 2 049 and 4 097 pairs, whose band is half their read, take the workgroup kernel)."""
    if first_k:
        monkeypatch.setenv("GC_ED_FIRST_K", first_k)
    _check(gca, oracle_distance, ring_pairs, f"first band {first_k}")


def test_team_boundaries(gca, oracle_distance, monkeypatch):
    """Reads of 1 345 and 2 049 bases: the 22nd and the 33rd unit, the first that a lane of a team of 21 and of 32 takes after its own; 1 400 at 50 % error."""
    rng = random.Random(43)
    pairs = []
    for length, rate in ((1345, 0.03), (1345, 0.2), (2049, 0.03), (2049, 0.2), (1400, 0.5)):
        read = _seq(rng, length)
        pairs.append((_columns(rng, _mutate(rng, read, rate), COLS - 1), read))
    _check(gca, oracle_distance, pairs)
    for first_k in ("100", "700", str(THIRD_KMAX - 1), str(HALF_KMAX - 1)):
        monkeypatch.setenv("GC_ED_FIRST_K", first_k)
        _check(gca, oracle_distance, pairs, f"first band {first_k}")


def _pair_at_distance(rng, oracle_distance, length, lo, hi):
    """A pair of `length` bases whose distance lies in [lo, hi]: substitutions at scattered places, as many as it takes."""
    a = _seq(rng, length)
    places = list(range(length))
    rng.shuffle(places)
    other = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}

    def with_substitutions(count):
        b = bytearray(a)
        for p in places[:count]:
            b[p] = other[a[p]][p % 3]
        return bytes(b)
    low, high = lo, min(length, 2 * hi)                                      # (at least one substitution per unit of distance)
    while low < high:                                                          # (the distance grows with the number of substitutions)
        mid = (low + high) // 2
        d = oracle_distance(with_substitutions(mid), a)
        if lo <= d <= hi:
            return with_substitutions(mid), a
        if d < lo:
            low = mid + 1
        else:
            high = mid
    raise AssertionError(f"no pair of {length} bases with a distance in [{lo}, {hi}]")


@pytest.mark.parametrize("limit", [THIRD_KMAX, HALF_KMAX])
def test_class_limits(gca, oracle_distance, monkeypatch, limit):
    """A 5 kb pair with the first band at limit - 1, the widest its team holds: a distance just below the band comes out of the first sweep, one just above it comes back
    through the rerun path (-2 from the team, the next kernel up) with the right value."""
    rng = random.Random(limit)
    below = _pair_at_distance(rng, oracle_distance, 5000, limit - 40, limit - 1)
    above = _pair_at_distance(rng, oracle_distance, 5000, limit, limit + 40)
    monkeypatch.setenv("GC_ED_FIRST_K", str(limit - 1))
    _check(gca, oracle_distance, [below, above, below], f"first band {limit - 1}")


def test_workgroup_kernel_with_a_ragged_last_group(gca, oracle_distance, monkeypatch):
    """A first band of half the read or more: every pair goes to the workgroup kernel (the whole matrix, C deltas per thread and step through LDS)."""
    rng = random.Random(47)
    pairs = []
    for length, rate, rem in ((65, 0.1, 1), (700, 0.15, COLS - 1), (3000, 0.05, 3), (3000, 0.4, 1)):
        read = _seq(rng, length)
        pairs.append((_columns(rng, _mutate(rng, read, rate), rem), read))
    pairs.append((b"ACGTNNRYACGT" * 30 + b"AC", b"ACGTNARYACGA" * 29))          # letters outside ACGT: groups of both kinds
    monkeypatch.setenv("GC_ED_FIRST_K", "30000")
    _check(gca, oracle_distance, pairs)


@pytest.mark.parametrize("first_k", [None, "1", "30000"])
def test_degenerate_sizes(gca, oracle_distance, monkeypatch, first_k):
    """Fewer columns than a group holds, fewer rows than a word, a band of one diagonal."""
    rng = random.Random(53)
    pairs = [(b"A", b"A"), (b"A", b"C"), (b"ACG", b"ACGT"), (_seq(rng, COLS - 1), _seq(rng, 63)), (_seq(rng, COLS + 1), _seq(rng, 5)), (_seq(rng, 2), _seq(rng, 200))]
    same = _seq(rng, 200)
    pairs += [(same, same), (same[:100] + b"N" + same[101:], same), (same[:COLS - 1], same[:COLS - 1])]
    if first_k:
        monkeypatch.setenv("GC_ED_FIRST_K", first_k)
    _check(gca, oracle_distance, pairs, f"first band {first_k}")
