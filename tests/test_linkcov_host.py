"""The link coverage core (csrc/hip/gc_coverage_links_core.hpp) as an ordinary program (tests/linkcov_host/linkcov_host_test.cpp), built with g++ once as it is and once
with -fsanitize=address,undefined and run directly: the canonical key and the search (a hairpin, the first and the last link, pairs that are no link), the traversal step
over 64 emulated lanes with the carry on the traces of link_coverage_model.cases(), and both line spellings with an empty name and a 20-digit count. What it prints is
held to the model here. Also here, without a device: the model's two statements agree, and the cases are what they claim."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import link_coverage_model as lm   # noqa: E402

NAMES = ["a", "", "c", "d", "a longer name e", "f"]       # the second segment has no name: it prints as its number, 1
LETTERS = ["A", "C" * 63, "ACGT" * 16, "N" + "RYKM" * 16, "G" * 130, "TTTTTTT"]
BASES = [3, 0, 64, 18446744073709551615, 130, 0]
BIG = 18446744073709551615                                # 20 digits
LINKS = lm.graph_links()
QUERIES = [lm.HAIRPIN, (9, 8), LINKS[0], LINKS[-1], (LINKS[0][1] ^ 1, LINKS[0][0] ^ 1), (LINKS[-1][1] ^ 1, LINKS[-1][0] ^ 1), (0, 4), (2, 10), (0, 0), (4294967295, 4294967294)]


def _hex(b):
    return b.hex() or "-"


def _build(tmp, sanitize):
    exe = str(tmp / ("linkcov_host_asan" if sanitize else "linkcov_host"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip")] + flags +
                   [os.path.join(ROOT, "tests", "linkcov_host", "linkcov_host_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _run(exe, tmp):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        f.write(f"G {len(NAMES)} " + " ".join(f"{_hex(n.encode())} {s} {b}" for n, s, b in zip(NAMES, LETTERS, BASES)) + "\n")
        f.write(f"L {len(LINKS)} " + " ".join(f"{u} {v}" for u, v in LINKS) + "\n")
        for u, v in QUERIES:
            f.write(f"K {u} {v}\n")
        for traces in list(lm.cases().values()) + [lm.every_case()]:
            for nodes, offsets in traces:
                f.write(f"T {len(nodes)} " + " ".join(f"{a} {b}" for a, b in zip(nodes, offsets)) + "\n")
            f.write("E\n")
        f.write(f"C 0 {BIG}\nC {len(LINKS) - 1} 10\nE\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def _check(lines):
    for (u, v), line in zip(QUERIES, lines):
        c = lm.canonical(u, v)
        assert line == f"K {c[0]} {c[1]} {LINKS.index(c) if c in LINKS else len(LINKS)}", (u, v)
    lines = lines[len(QUERIES):]
    sets = list(lm.cases().items()) + [("every case", lm.every_case()), ("a 20-digit count", None)]
    assert len(lines) == 5 * len(sets)
    for k, (name, traces) in enumerate(sets):
        counts = lm.from_traces(traces) if traces is not None else {LINKS[0]: BIG, LINKS[-1]: 10}
        whole = lm.gfa_text(NAMES, LETTERS, BASES, LINKS, counts).decode().splitlines(keepends=True)[1:]
        kept = lm.gfa_text(NAMES, LETTERS, BASES, LINKS, counts, supported_only=True).decode().splitlines(keepends=True)[1:]
        part = lambda rows, kind: _hex("".join(r for r in rows if r[0] == kind).encode())   # noqa: E731
        assert lines[5 * k:5 * k + 5] == ["T " + _hex(lm.link_table(NAMES, LINKS, counts)), "S " + part(whole, "S"), "L " + part(whole, "L"), "s " + part(kept, "S"), "l " + part(kept, "L")], name


def test_the_cases_cover_what_they_claim():
    cases = lm.cases()
    first = lambda t: [i for i in range(1, len(t[0])) if t[0][i] != t[0][i - 1]]   # noqa: E731
    assert first(cases["a traversal at cell 1"][0]) == [1] and first(cases["a traversal at cell 63"][0]) == [63]
    assert first(cases["a traversal at cell 64, over the carry"][0]) == [64] and first(cases["a traversal at cell 65"][0]) == [65]
    assert [len(t[0]) for t in cases["one cell"] + cases["65 cells and no traversal"]] == [1, 65] and lm.from_traces(cases["one cell"] + cases["65 cells and no traversal"]) == {}
    nodes, offsets = cases["a traversal right after insertions"][0]
    assert len({(nodes[i], offsets[i]) for i in range(12, 24)}) == 1 and offsets[12] == 62 and (nodes[24], offsets[24]) == (4, 0)
    nodes, offsets = cases["insertions over the chunk boundary, then a traversal"][0]
    assert len({(nodes[i], offsets[i]) for i in range(59, 70)}) == 1 and offsets[59] == 63 and (nodes[70], offsets[70]) == (6, 0)
    assert lm.from_traces(cases["one link on both strands"]) == {(2, 4): 2}
    assert lm.from_traces(cases["two alignments share a link"]) == {(4, 6): 2, (6, 8): 1}
    assert lm.from_traces(cases["the hairpin"]) == {lm.HAIRPIN: 1} and lm.canonical(9, 8) == (9, 8) and lm.canonical(*lm.HAIRPIN) == lm.HAIRPIN
    assert lm.from_traces(cases["the side road"]) == {(2, 11): 2, (7, 10): 2}
    assert set(lm.from_traces(lm.every_case())) == set(LINKS) and len(LINKS) == 7          # every link of the graph is walked by some case
    # every traversal leaves at the last base and enters at offset 0, along a link: what gc_coverage_add_traces accepts
    for nodes, offsets in lm.every_case():
        for i in first((nodes, offsets)):
            assert offsets[i - 1] == lm.LENGTHS[nodes[i - 1] // 2] - 1 and offsets[i] == 0 and lm.canonical(nodes[i - 1], nodes[i]) in LINKS


def test_traces_and_gaf_lines_state_the_same_counts(tmp_path):
    """The model's two statements on the same alignments: the node changes of the traces, and the steps of the GAF path the traces spell."""
    gfa = str(tmp_path / "g.gfa")
    lm.write_graph(gfa)
    ids = lm.segment_ids_of_gfa(gfa)
    assert ids == {n: i for i, n in enumerate(lm.NAMES)} and lm.links_of_gfa(gfa) == LINKS
    gaf = []
    for nodes, _ in lm.every_case():
        steps = [n for i, n in enumerate(nodes) if i == 0 or n != nodes[i - 1]]
        gaf.append("read\t1\t0\t1\t+\t" + "".join("<>"[1 - (n & 1)] + lm.NAMES[n // 2] for n in steps) + "\t1\t0\t1\t1\t1\t60")
    assert lm.from_gaf("\n".join(gaf) + "\n", ids) == lm.from_traces(lm.every_case())
    text = lm.gfa_text(lm.NAMES, ["A" * n for n in lm.LENGTHS], [1] * 6, LINKS, lm.from_traces(lm.every_case()))
    segments, links = lm.read_tagged_gfa(text)
    assert list(segments) == lm.NAMES and [s[1] for s in segments.values()] == lm.LENGTHS and len(links) == 7 and links[0] == ("a", "+", "b", "+", "0M", 2)


def test_keys_lanes_and_lines_on_the_host_equal_the_model(tmp_path):
    _check(_run(_build(tmp_path, False), tmp_path))


def test_keys_lanes_and_lines_under_the_address_and_undefined_sanitizers(tmp_path):
    """The same cases through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _check(_run(_build(tmp_path, True), tmp_path))
