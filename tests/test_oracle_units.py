"""Pins the oracle's leaf functions against the reference's own sources compiled unmodified
(oracle/_ref/libref_units.so = WordSlice.h, AlignmentCorrectnessEstimation.cpp, edlib).

Where oracle/_ref is not built (its sources are not part of this repository), the reference's outputs for the same seeded
inputs come from tests/golden/ref_units.expected.npz, which tests/golden/make_ref_units_golden.py recorded from oracle/_ref;
where it is built, the live outputs are compared with the oracle and with that recording."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

from oracle import RefUnits, load_oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
REF_GOLDEN = os.path.join(HERE, "golden", "ref_units.expected.npz")


def live_ref():
    """RefUnits when oracle/_ref/libref_units.so is built (or can be), else None."""
    try:
        return RefUnits()
    except (FileNotFoundError, OSError):
        return None


def reference(name):
    """The reference units' outputs for one test's inputs (RECORDED[name]): live when the units are built - and then they must equal the
    recording - else the recording."""
    recorded = np.load(REF_GOLDEN)[name]
    ref = live_ref()
    if ref is None:
        return recorded
    got = RECORDED[name](ref)
    assert np.array_equal(got, recorded), f"{name}: the reference units' outputs differ from {os.path.basename(REF_GOLDEN)}"
    return got


def digest(*arrays):
    """16 bytes that stand for the exact bytes of `arrays` (a case's output where it is a whole series)."""
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def random_column(rng, flat=False):
    """A valid column: VP & VN == 0, plus a scoreEnd."""
    style = rng.random()
    if flat or style < 0.1:
        vp, vn = 0, 0
    elif style < 0.2:
        vp, vn = (1 << 64) - 1, 0
    elif style < 0.3:
        vp, vn = 0, (1 << 64) - 1
    else:
        p = rng.choice([0.05, 0.2, 0.5])
        vp = vn = 0
        for i in range(64):
            x = rng.random()
            if x < p:
                vp |= 1 << i
            elif x < 2 * p:
                vn |= 1 << i
    return vp, vn, rng.randint(0, 300)


def perturb(rng, col):
    """A column that differs from `col` in a few rows (the common case inside the band)."""
    vp, vn, s = col
    for _ in range(rng.randint(0, 4)):
        i = rng.randrange(64)
        vp &= ~(1 << i)
        vn &= ~(1 << i)
        x = rng.random()
        if x < 0.33:
            vp |= 1 << i
        elif x < 0.66:
            vn |= 1 << i
    return vp, vn, s + rng.randint(-2, 2)


def values(col):
    vp, vn, s = col
    before = s - bin(vp).count("1") + bin(vn).count("1")
    out = [before]
    for i in range(64):
        out.append(out[-1] + ((vp >> i) & 1) - ((vn >> i) & 1))
    return out


@pytest.fixture(scope="module")
def ora():
    return load_oracle_lib()


def merge_cases():
    rng = random.Random(1)
    cases = []
    for it in range(20000):
        a = random_column(rng)
        b = perturb(rng, a) if it % 2 else random_column(rng)
        # the reference requires |score difference| small enough for its loop; keep columns within 64 of each other
        cases.append((a, b))
    return cases


def merge_outputs(fn, cases):
    """fn = gco_merge / ref_merge: [(VP, VN, scoreEnd)] of every case."""
    u64, i32 = C.c_uint64, C.c_int32
    out = np.zeros((len(cases), 3), dtype=np.int64)
    for k, (a, b) in enumerate(cases):
        vp, vn, s = u64(), u64(), i32()
        fn(*a, *b, C.byref(vp), C.byref(vn), C.byref(s))
        out[k] = (np.uint64(vp.value).view(np.int64), np.uint64(vn.value).view(np.int64), s.value)
    return out


def test_merge_matches_reference_and_pointwise_min(ora):
    cases = merge_cases()
    got = merge_outputs(ora.gco_merge, cases)
    want = reference("merge")
    for k, (a, b) in enumerate(cases):
        assert np.array_equal(got[k], want[k]), (a, b)
        vp, vn = (int(x) & ((1 << 64) - 1) for x in got[k][:2])
        mins = [min(x, y) for x, y in zip(values(a), values(b))]
        assert values((vp, vn, int(got[k][2]))) == mins


def score_cases():
    rng = random.Random(2)
    cases = []
    for it in range(20000):
        a = random_column(rng)
        b = perturb(rng, a) if it % 2 else random_column(rng)
        cases.append((a, b, rng.randrange(64)))
    return cases


def score_outputs(lib, prefix, cases):
    """[(changedMinScore(a, b), scoreBeforeStart(a), getValue(a, row))] of every case."""
    changed, before, value = (getattr(lib, prefix + n) for n in ("changed_min_score", "score_before_start", "get_value"))
    return np.array([(changed(*a, *b), before(*a), value(*a, row)) for a, b, row in cases], dtype=np.int64)


def test_changed_min_score_get_value_before_start(ora):
    cases = score_cases()
    got = score_outputs(ora, "gco_", cases)
    want = reference("scores")
    for k, (a, b, row) in enumerate(cases):
        assert got[k][0] == want[k][0], (a, b)
        assert got[k][1] == want[k][1]
        assert got[k][2] == want[k][2] == values(a)[row + 1]


def test_myers_step_is_the_cell_recurrence(ora):
    """getNextSlice against the plain DP recurrence (the reference's assertSliceCorrectness twin,
    src/GraphAlignerBitvectorCommon.h:812-826)."""
    rng = random.Random(3)
    u64, i32 = C.c_uint64, C.c_int32
    for _ in range(5000):
        old = random_column(rng)
        eq = rng.getrandbits(64)
        hin = rng.choice([(0, 0), (1, 0), (0, 1)])
        ovp, ovn, os_, hp, hn = u64(), u64(), i32(), u64(), u64()
        ora.gco_next_slice(eq, *old, hin[0], hin[1], C.byref(ovp), C.byref(ovn), C.byref(os_), C.byref(hp), C.byref(hn))
        o = values(old)
        n = values((ovp.value, ovn.value, os_.value))
        assert n[0] == o[0] + hin[0] - hin[1]
        for i in range(64):
            want = min(n[i] + 1, o[i + 1] + 1, o[i] + (0 if (eq >> i) & 1 else 1))
            assert n[i + 1] == want
        assert hp.value - hn.value == n[64] - o[64]


def correctness_cases():
    rng = random.Random(4)
    cases = []
    for _ in range(200):
        n = rng.randint(1, 200)
        lo, hi = rng.choice([(0, 8), (5, 20), (20, 40), (0, 70)])
        cases.append(np.array([rng.randint(lo, hi) for _ in range(n)], dtype=np.int32))
    return cases


def correctness_series(fn, mm):
    n = len(mm)
    c, w, f = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    fn(mm.ctypes.data, n, c.ctypes.data, w.ctypes.data, f.ctypes.data)
    return c, w, f


def test_correctness_hmm_matches_reference(ora):
    cases = correctness_cases()
    # bit-exact doubles: a case's three series enter its digest as bytes
    want = reference("correctness")
    for k, mm in enumerate(cases):
        assert np.array_equal(digest(*correctness_series(ora.gco_correctness_series, mm)), want[k]), mm.tolist()


def edit_distance_cases():
    rng = random.Random(5)
    cases = []
    for _ in range(300):
        la = rng.choice([1, 5, 63, 64, 65, 130, 500])
        a = "".join(rng.choice("ACGT") for _ in range(la))
        b = list(a)
        for _ in range(rng.randint(0, max(1, la // 5))):
            op = rng.random()
            i = rng.randrange(len(b)) if b else 0
            if op < 0.4 and b:
                b[i] = rng.choice("ACGT")
            elif op < 0.7 and b:
                del b[i]
            else:
                b.insert(i, rng.choice("ACGT"))
        b = "".join(b) or "A"
        cases.append((a.encode(), b.encode()))
    return cases


def test_edit_distance_matches_edlib(ora):
    cases = edit_distance_cases()
    want = reference("edit_distance")
    for (a, b), w in zip(cases, want):
        assert ora.gco_edit_distance(a, len(a), b, len(b)) == w, (a, b)


# ---- edlib PATH mode (src/Aligner.cpp:845) and the E-value (src/EValue.cpp) ----------------------------------------

def _mut(rng, s, rate):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if rng.random() < rate / 3:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _path_cases(rng):
    """(query = path letters, target = read): the shapes the chained alignment meets - similar strings, a path that covers
    only the left / right / middle part of the read (stitching keeps the longest piece), a path with a stretch the read
    lacks, unrelated strings, repeats (many equally good alignments), IUPAC letters, tiny and empty sides."""
    for n in (0, 1, 2, 63, 64, 65, 200):
        q = _rand(rng, n)
        yield q, _mut(rng, q, 0.15)
        yield q, _rand(rng, rng.randint(0, 130))
    for _ in range(30):
        q = _rand(rng, rng.randint(100, 900))
        yield q, _mut(rng, q, rng.choice([0.02, 0.1, 0.3]))
        yield q, _rand(rng, 400) + _mut(rng, q, 0.1)
        yield q, _mut(rng, q, 0.1) + _rand(rng, 350)
        yield q, _rand(rng, 150) + _mut(rng, q, 0.08) + _rand(rng, 220)
        yield q, _mut(rng, q[:len(q) // 3], 0.1) + _mut(rng, q[2 * len(q) // 3:], 0.1)
    for _ in range(10):
        unit = _rand(rng, rng.randint(1, 7))
        q = (unit * 200)[:rng.randint(50, 600)]
        yield q, _mut(rng, q, 0.1)
        yield _rand(rng, 300, b"AC"), _rand(rng, 280, b"AC")
    q = _rand(rng, 500, b"ACGTNRY")
    yield q, _mut(rng, q, 0.1)
    # above edlib's 1 MB limit: Hirschberg splits (edlib/src/edlib.cpp:1204-1212), incl. splits on the matrix border
    for qn in (1500, 2600, 4200):
        q = _rand(rng, qn)
        yield q, _mut(rng, q, 0.12)
        yield q, _rand(rng, 3000) + _mut(rng, q, 0.1)
        yield q, _mut(rng, q, 0.1) + _rand(rng, 3300)
        yield q, _rand(rng, 2000) + _mut(rng, q, 0.08) + _rand(rng, 2500)
        yield q, _mut(rng, q[:qn // 3], 0.1) + _mut(rng, q[2 * qn // 3:], 0.1)
        yield q[:300], _rand(rng, 9000)
        yield (b"ACG" * 2000)[:qn], _mut(rng, (b"ACG" * 2000)[:qn], 0.05)


def edit_path_record(d, ops):
    """One case of edlib's PATH output as recorded: distance, op count, digest of the op string."""
    return np.concatenate([np.array([d, len(ops)], dtype=np.int64).view(np.uint8), digest(np.asarray(ops, dtype=np.uint8))])


def test_edit_path_matches_edlib_op_for_op():
    """oracle/edlib_path.hpp against the real edlib (oracle/_ref): same distance, same op string, same "no alignment" cases."""
    from oracle.binding import oracle_edit_path
    cases = list(_path_cases(random.Random(2024)))
    want = reference("edit_path")
    n = hirschberg = 0
    for (q, t), w in zip(cases, want):
        got_d, got_ops = oracle_edit_path(q, t)
        want_d, want_len = w[:16].view(np.int64)
        assert got_d == want_d, (len(q), len(t))
        assert np.array_equal(edit_path_record(got_d, got_ops), w), (len(q), len(t), want_d)
        if want_len:
            # an op string is an alignment: it consumes both strings and costs the distance
            assert np.sum(got_ops != 2) == len(q) and np.sum(got_ops != 1) == len(t) and np.sum(got_ops != 0) == want_d
        n += 1
        hirschberg += (20 * ((len(q) + 63) // 64) + 8) * len(t) >= 1 << 20
    assert n > 200 and hirschberg >= 15


def test_edit_path_edges_match_edlib_op_for_op():
    """oracle/edlib_path.hpp against the real edlib on tests/edit_path_cases.py: nearly identical strings above the 1 MB limit (the optimal split on the edge of a band a few
    blocks wide - where the restatement once narrowed the band after the last column and answered "no alignment"), either side of the limit, tall thin leaves, column counts at
    1 023 .. 8 194 and letters outside ACGT. Same distance, same op count, same ops; and every pair, none of which has an empty side, gets an alignment."""
    from edit_path_cases import assert_is_alignment, edit_path_cases, is_split
    from oracle.binding import oracle_edit_path
    cases = edit_path_cases()
    want = reference("edit_path_edges")
    assert len(want) == len(cases)
    blocks = {}
    wrong = []
    for (name, q, t), w in zip(cases, want):
        got_d, got_ops = oracle_edit_path(q, t)
        want_d, want_len = (int(x) for x in w[:16].view(np.int64))
        if got_d != want_d or len(got_ops) != want_len or not np.array_equal(edit_path_record(got_d, got_ops), w):
            wrong.append((name, len(q), len(t), got_d, want_d, len(got_ops), want_len))
            continue
        assert_is_alignment(q, t, want_d, got_ops, name)
        blocks.setdefault(name.split("/")[0], []).append(is_split(q, t))
    assert not wrong, f"{len(wrong)} of {len(cases)} (name, Q, T, distance, edlib's, ops, edlib's): {wrong[:12]}"
    assert {b: len(v) for b, v in blocks.items()} == {"near": 96, "limit": 8, "strips": 3, "rings": 14, "letters": 4}
    assert all(blocks["near"]) and blocks["strips"] == [False, False, True] and all(blocks["rings"]) and all(blocks["letters"])   # (10 000 x 500: halves of 250 columns)
    assert blocks["limit"] == [False, True] * 4


def evalue_cases():
    rng = random.Random(7)
    cases = []
    for _ in range(300):
        ident = rng.choice([0.7, 0.5, 0.66, 0.9, rng.uniform(0.05, 0.95)])
        db, q = rng.randint(1, 10**10), rng.randint(1, 10**5)
        length = rng.randint(0, 60000)
        edits = rng.randint(0, max(1, length))
        cases.append((ident, db, q, length, edits))
    return cases


def test_evalue_matches_reference_bitwise():
    from oracle.binding import oracle_evalue
    cases = evalue_cases()
    want = reference("evalue")
    for c, w in zip(cases, want):
        got = oracle_evalue(*c)
        assert w.tobytes() == got.tobytes(), (c, w.view(np.float64), got)


# seeded inputs -> the reference units' outputs, as tests/golden/make_ref_units_golden.py records them
RECORDED = {
    "merge": lambda ref: merge_outputs(ref.lib.ref_merge, merge_cases()),
    "scores": lambda ref: score_outputs(ref.lib, "ref_", score_cases()),
    "correctness": lambda ref: np.array([digest(*correctness_series(ref.lib.ref_correctness_series, mm)) for mm in correctness_cases()]),
    "edit_distance": lambda ref: np.array([ref.lib.ref_edit_distance(a, len(a), b, len(b)) for a, b in edit_distance_cases()], dtype=np.int64),
    "edit_path": lambda ref: np.array([edit_path_record(*ref.edit_path(q, t)) for q, t in _path_cases(random.Random(2024))]),
    "evalue": lambda ref: np.array([ref.evalue(*c) for c in evalue_cases()]).view(np.uint64),
    "edit_path_edges": lambda ref: _edit_path_edges(ref),
}


def _edit_path_edges(ref):
    from edit_path_cases import edit_path_cases
    return np.array([edit_path_record(*ref.edit_path(q, t)) for _, q, t in edit_path_cases()])
