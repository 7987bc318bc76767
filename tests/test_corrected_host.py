"""The corrected reads' host/device core (csrc/hip/gc_corrected_core.hpp) as an ordinary program (tests/corrected_host/corrected_host_test.cpp), built with g++ once as it
is and once with -fsanitize=address,undefined and run directly. The program runs the kernel's loop over 64 emulated lanes - the keep flag of lane 0 from the previous
chunk's last cell, a keep mask, the rank below the lane - on traces of 1, 2, 63, 64, 65, 128, 129 and 200 cells with insertion and deletion runs laid across the chunk
boundaries, compares with a plain loop itself, and prints the pieces; the records come from the host's assembly. Both are held to tests/corrected_model.py here."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corrected_model as cm   # noqa: E402

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)
TABLE = b"NACMGRSVTWYHKDBN"
NODE_LETTERS = 100                      # letters per node of the walk: node changes at cells 100, 200 of a walk without insertions, elsewhere with them


def letter(node, offset):
    s = (node * 5 + offset) & 15
    return TABLE[s:s + 1]


VARIANTS = {
    "matches and deletions only": lambda n: set(),                                                   # every cell advances in the graph: all kept
    "insertion runs across the chunk boundaries": lambda n: set(range(61, 68)) | set(range(125, 132)) | set(range(190, 200)),
    "an insertion in lane 0 of a chunk": lambda n: {64, 128},                                       # its predecessor is the carried cell
    "an insertion in lane 63 of a chunk": lambda n: {63, 127},
    "one position throughout": lambda n: set(range(1, n)),                                          # cell 0 alone is kept
    "every other cell": lambda n: set(range(1, n, 2)),
    "deletion runs around insertions at the boundaries": lambda n: {62, 66, 126, 130},
}
KEPT_REPEATS = {64, 128}                # variant "a repeated position behind a node switch": cells 63 / 127 are flagged, cells 64 / 128 repeat them and are kept


def make_trace(n, repeats, flagged_before=()):
    """A walk of n cells from (4, 0): a cell in `repeats` stands where the one before it does (an insertion), every other advances by one letter, into the next node
    (id + 2) after NODE_LETTERS letters with the cell before it flagged. flagged_before: repeats whose predecessor is flagged nodeSwitch all the same."""
    cells, node, offset = [], 4, 0
    for i in range(n):
        if i > 0 and i not in repeats:
            offset += 1
            if offset == NODE_LETTERS:
                node, offset = node + 2, 0
                cells[-1] = (cells[-1][0], cells[-1][1], 1)
        if i in flagged_before and i > 0:
            cells[-1] = (cells[-1][0], cells[-1][1], 1)
        cells.append((node, offset, 0))
    return cells


def traces():
    out = []
    for n in LENGTHS:
        for name, repeats in VARIANTS.items():
            out.append((f"{n} cells, {name}", make_trace(n, {i for i in repeats(n) if i < n})))
        out.append((f"{n} cells, a repeated position behind a node switch", make_trace(n, {i for i in KEPT_REPEATS if i < n}, flagged_before=KEPT_REPEATS)))
    return out


RAW = b"acgtNNRYacgtACGTacgt"
RECORDS = [
    # (max_overlap, id, raw, corrections)
    (0, b"r1 with a description", RAW, [(2, 6, b"ggtt"), (6, 10, b"AaCc"), (14, 16, b"TT")]),          # a gap, an abutting piece, a tail
    (0, b"r2", RAW, [(0, 8, b"ACGTACGT"), (5, 12, b"CGTAAAA")]),                                      # overlapping: nothing trimmed
    (0, b"r3", RAW, [(0, 12, b"A" * 12), (4, 9, b"CCCCC"), (10, 20, b"G" * 10)]),                      # currentEnd moves backwards
    (0, b"r4", RAW, []),                                                                               # no alignment
    (0, b"r5", b"ACNRYKacgu", [(3, 5, b"rn")]),
    (3, b"r6", RAW, [(0, 8, b"ACGTACGT"), (5, 12, b"CGTAAAA")]),                                      # getLongestOverlap with maxOverlap > 0
    (5, b"r7", RAW, [(0, 7, b"CCGATTA"), (3, 8, b"TTAGG"), (6, 9, b"GGA")]),
    (0, b"", b"", []),
]


def _hex(b):
    return b.hex() or "-"


def _unhex(s):
    return b"" if s == "-" else bytes.fromhex(s)


def _build(tmp, sanitize):
    exe = str(tmp / ("corrected_host_asan" if sanitize else "corrected_host"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip")] + flags +
                   [os.path.join(ROOT, "tests", "corrected_host", "corrected_host_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _run(exe, tmp):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for _, cells in traces():
            f.write(f"T {len(cells)} " + " ".join(f"{a} {b} {c}" for a, b, c in cells) + "\n")
        for max_overlap, name, raw, corrections in RECORDS:
            f.write(f"B {max_overlap} {_hex(name)} {_hex(raw)} {len(corrections)} " + " ".join(f"{s} {e} {_hex(p)}" for s, e, p in corrections) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def _check(lines):
    cases = traces()
    assert len(lines) == len(cases) + len(RECORDS)
    for (name, cells), line in zip(cases, lines):
        assert line == "T " + cm.add_corrected(cells, letter).decode(), name
    for (max_overlap, name, raw, corrections), line in zip(RECORDS, lines[len(cases):]):
        kind, record, clipped = line.split()
        assert kind == "B"
        assert _unhex(record) == cm.corrected_record(name, raw, corrections, max_overlap), name
        assert _unhex(clipped) == b"".join(cm.clipped_records(name, corrections)), name


def test_the_traces_cover_what_they_claim():
    by_name = dict(traces())
    assert len(cm.add_corrected(by_name["200 cells, matches and deletions only"], letter)) == 200
    assert {c[0] for c in by_name["200 cells, matches and deletions only"]} == {4, 6}                 # a node change, its last cell flagged
    assert by_name["200 cells, matches and deletions only"][99][2] == 1
    assert len(cm.add_corrected(by_name["129 cells, one position throughout"], letter)) == 1
    plain, kept = by_name["65 cells, an insertion in lane 0 of a chunk"], by_name["65 cells, a repeated position behind a node switch"]
    assert plain[64][:2] == plain[63][:2] and plain[63][2] == 0 and len(cm.add_corrected(plain, letter)) == 64
    assert kept[64][:2] == kept[63][:2] and kept[63][2] == 1 and len(cm.add_corrected(kept, letter)) == 65
    run = by_name["129 cells, insertion runs across the chunk boundaries"]
    assert all(run[i][:2] == run[60][:2] for i in range(61, 68)) and all(run[i][:2] == run[124][:2] for i in range(125, 129))
    letters = set()
    for _, cells in traces():
        letters |= set(cm.add_corrected(cells, letter))
    assert letters == set(TABLE)                                                                       # every entry of the letter table


def test_lanes_and_records_on_the_host_equal_the_model(tmp_path):
    _check(_run(_build(tmp_path, False), tmp_path))


def test_lanes_and_records_under_the_address_and_undefined_sanitizers(tmp_path):
    """The same cases through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _check(_run(_build(tmp_path, True), tmp_path))
