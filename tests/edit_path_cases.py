"""Seeded (query, target) pairs for the edit path (edlibAlign(query, target, NW, PATH)) placed on the fixed points of oracle/edlib_path.hpp and of k_edit_path
(csrc/hip/gc_edpath.hip), shared by tests/test_oracle_units.py, tests/test_edit_path_edges_gpu.py and tests/golden/make_ref_units_golden.py. Needs no GPU.

query = rows = path letters, target = columns = read. A problem is traced back directly while (20 blocks + 8) columns < 2**20 (blocks = 64-row words of the query), else it
is cut at the middle column. The blocks:
  near     nearly identical strings above that limit, both orders: the distance is 0-5, so edlib's band is a few blocks wide and the optimal split sits on its edge
  limit    the largest directly traced problem and the smallest split one at 1, 2, 6 and 65 blocks (6 blocks x 8 192 columns is exactly 2**20: split)
  strips   directly traced problems of more than 64 blocks: the kernel stores and walks back across strips of 64 blocks
  rings    two strips (the carries between them in use) with the sweeps' column counts on either side of the kernel's ring marks at 1 024, 2 048 and 4 096 columns,
           and 8 193 rows against 63 and 64 columns more
  letters  IUPAC codes (compared one by one, in reversed halves and lower strips too) and upper against lower case, both orders
"""
import random

SEED = 20260
NEAR_LENGTHS = (4095, 4096, 4097, 8192, 8193, 10000)
NEAR_KINDS = ("identical", "one_more_at_end", "one_more_at_start", "one_deleted_at_third", "inserted_at_quarter_deleted_at_three_quarters", "two_more_at_both_ends",
              "first_three_removed", "five_substitutions")
RING_TARGETS = (2047, 2048, 2049, 2050, 4095, 4096, 4097, 4098, 8191, 8192, 8193, 8194)
IUPAC = b"ACGTNRYKMSWBDHV"


def is_split(q, t):
    """edlib cuts the problem at the middle column instead of tracing it back directly (edlib/src/edlib.cpp:1204-1212)."""
    return (20 * ((len(q) + 63) // 64) + 8) * len(t) >= 1 << 20


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _other(rng, ch, alphabet=b"ACGT"):
    return rng.choice(bytes(c for c in alphabet if c != ch))


def _mutate(rng, s, rate, alphabet=b"ACGT"):
    """Substitutions, deletions and insertions, a third of `rate` each."""
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(_other(rng, ch, alphabet) if x < 2 * rate / 3 else ch)
        if rng.random() < rate / 3:
            out.append(rng.choice(alphabet))
    return bytes(out)


def _fit(rng, s, n):
    """s cut, or padded with random letters, to n letters."""
    return s[:n] + _rand(rng, max(0, n - len(s)))


def _near(rng, q, kind):
    n = len(q)
    if kind == "identical":
        return q
    if kind == "one_more_at_end":
        return q + _rand(rng, 1)
    if kind == "one_more_at_start":
        return _rand(rng, 1) + q
    if kind == "one_deleted_at_third":
        return q[:n // 3] + q[n // 3 + 1:]
    if kind == "inserted_at_quarter_deleted_at_three_quarters":
        return q[:n // 4] + _rand(rng, 1) + q[n // 4:3 * n // 4] + q[3 * n // 4 + 1:]
    if kind == "two_more_at_both_ends":
        return _rand(rng, 2) + q + _rand(rng, 2)
    if kind == "first_three_removed":
        return q[3:]
    assert kind == "five_substitutions"
    t = bytearray(q)
    for i in range(5):
        at = (2 * i + 1) * n // 10 + rng.randrange(-50, 50)
        t[at] = _other(rng, t[at])
    return bytes(t)


def edit_path_cases():
    """[(name, query, target)], always the same. A name is block/shape/...; the pairs given in both orders end in /fwd and /swapped."""
    out = []

    def both(name, q, t):
        out.append((name + "/fwd", q, t))
        out.append((name + "/swapped", t, q))

    for n in NEAR_LENGTHS:
        rng = random.Random(SEED * 100003 + n)
        q = _rand(rng, n)
        for kind in NEAR_KINDS:
            both(f"near/{n}/{kind}", q, _near(rng, q, kind))

    rng = random.Random(SEED + 1)
    for qn, below in ((64, 37449), (128, 21845), (4097, 801), (350, 8191)):
        for tn in (below, below + 1):
            q = _rand(rng, qn)
            if tn > qn:   # a short path somewhere inside a long read
                at = tn // 3
                t = _rand(rng, at) + _mutate(rng, q, 0.1)
                t = _fit(rng, t, tn)
            else:         # a short read that spells a slice of a long path
                t = _fit(rng, _mutate(rng, q[qn // 2:qn // 2 + tn], 0.1), tn)
            out.append((f"limit/{qn}x{tn}", q, t))

    rng = random.Random(SEED + 2)
    for qn, tn in ((4097, 801), (10000, 300), (10000, 500)):
        q = _rand(rng, qn)
        out.append((f"strips/{qn}x{tn}", q, _fit(rng, _mutate(rng, q[qn // 2:qn // 2 + tn], 0.1), tn)))

    rng = random.Random(SEED + 3)
    for tn in RING_TARGETS:
        q = _rand(rng, 4200)
        out.append((f"rings/4200x{tn}", q, _fit(rng, _mutate(rng, q, 0.05), tn)))
    for extra in (63, 64):
        q = _rand(rng, 8193)
        out.append((f"rings/8193x{8193 + extra}", q, _fit(rng, _mutate(rng, q, 0.05), 8193 + extra)))

    rng = random.Random(SEED + 4)
    q = _rand(rng, 8193, IUPAC)
    both("letters/iupac_8193", q, _mutate(rng, q, 0.1, IUPAC))
    q = _rand(rng, 4200)
    both("letters/lower_case_4200", q, _mutate(rng, q, 0.05).lower())
    return out


def assert_is_alignment(q, t, distance, ops, note=""):
    """A non-empty pair has an op string (0 match, 1 query letter alone, 2 target letter alone, 3 mismatch) that consumes both strings, calls a match a match and a
    mismatch a mismatch, and costs the distance."""
    import numpy as np
    ops = np.asarray(ops, dtype=np.uint8)
    assert len(ops) > 0, f"{note}: no alignment"
    assert ops.max() <= 3, note
    assert int(np.sum(ops != 2)) == len(q) and int(np.sum(ops != 1)) == len(t), f"{note}: the ops do not consume both strings"
    assert int(np.sum(ops != 0)) == distance, f"{note}: the ops cost {int(np.sum(ops != 0))}, the distance is {distance}"
    diagonal = (ops == 0) | (ops == 3)
    row = np.cumsum(ops != 2)[diagonal] - 1
    col = np.cumsum(ops != 1)[diagonal] - 1
    same = np.frombuffer(q, dtype=np.uint8)[row] == np.frombuffer(t, dtype=np.uint8)[col]
    assert np.array_equal(same, ops[diagonal] == 0), f"{note}: a match op on unequal letters or a mismatch op on equal ones"


def gpu_subset(cases):
    """Indices of the cases the device test runs: everything but the near-identical lengths other than 4 096, 4 097 and 8 193."""
    return [i for i, (name, _, _) in enumerate(cases) if not name.startswith("near/") or name.split("/")[1] in ("4096", "4097", "8193")]
