"""Link coverage (--link-coverage-out / --coverage-gfa-out / --supported-subgraph-out; include/graphchainer_amd.h has the definition), stated twice in plain Python:

  from_traces   node changes of traces in output coordinates: cell i > 0 is a traversal iff node[i] != node[i-1]; it walks (node[i-1], node[i])
  from_gaf      consecutive steps of the path field of every GAF line the same run writes (>name forward, <name reverse)

Both count canonical pairs: the mate of (u, v) is (v ^ 1, u ^ 1), the canonical form the lexicographically smaller of the two. links_of_gfa is the graph's link set
from its L lines (the numbering of the handle), link_table / gfa_text the writers, read_tagged_gfa the reader of what --coverage-gfa-out writes."""
import re
from collections import Counter

HEAD = "#from\tfrom_orient\tto\tto_orient\ttraversals\n"


def canonical(u, v):
    return min((int(u), int(v)), (int(v) ^ 1, int(u) ^ 1))


def from_traces(traces):
    """traces: (nodes, offsets) each -> Counter {canonical (u, v): traversals}"""
    counts = Counter()
    for nodes, _ in traces:
        for i in range(1, len(nodes)):
            if nodes[i] != nodes[i - 1]:
                counts[canonical(nodes[i - 1], nodes[i])] += 1
    return counts


def gaf_steps(path_field, segment_ids):
    """'>s1<s2' -> bigraph ids"""
    steps = re.findall(r"([<>])([^<>]+)", path_field)
    assert "".join(a + b for a, b in steps) == path_field
    return [2 * segment_ids[name] + (1 if orient == "<" else 0) for orient, name in steps]


def from_gaf(text, segment_ids):
    counts = Counter()
    for line in text.splitlines():
        if not line:
            continue
        steps = gaf_steps(line.split("\t")[5], segment_ids)
        for u, v in zip(steps, steps[1:]):
            counts[canonical(u, v)] += 1
    return counts


def segment_ids_of_gfa(path):
    """{name: internal segment number}: the order in which the GFA first names a segment, in an S line or in an L line."""
    index = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            index.setdefault(f[1], len(index))
        elif f[0] == "L":
            index.setdefault(f[1], len(index))
            index.setdefault(f[3], len(index))
    return index


def links_of_gfa(path):
    """The graph's links: sorted distinct canonical pairs of its L lines."""
    ids = segment_ids_of_gfa(path)
    links = set()
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "L":
            links.add(canonical(2 * ids[f[1]] + (f[2] == "-"), 2 * ids[f[3]] + (f[4] == "-")))
    return sorted(links)


def shown(names, node):
    return (str(names[node // 2]) if str(names[node // 2]) != "" else str(node // 2)), "+-"[node & 1]


def link_row(names, link):
    (a, ao), (b, bo) = shown(names, link[0]), shown(names, link[1])
    return f"{a}\t{ao}\t{b}\t{bo}"


def link_table(names, links, counts):
    return (HEAD + "".join(f"{link_row(names, k)}\t{counts.get(k, 0)}\n" for k in links)).encode()


def gfa_text(names, letters, bases, links, counts, supported_only=False):
    """The tagged GFA as the writers spell it; letters: one upper-case string per segment, bases: the segment table's counts."""
    out = ["H\tVN:Z:1.0\n"]
    for i, name in enumerate(names):
        if not supported_only or int(bases[i]) > 0:
            out.append(f"S\t{shown(names, 2 * i)[0]}\t{letters[i]}\tLN:i:{len(letters[i])}\tRC:i:{int(bases[i])}\n")
    for k in links:
        if not supported_only or counts.get(k, 0) > 0:
            out.append(f"L\t{link_row(names, k)}\t0M\tRC:i:{counts.get(k, 0)}\n")
    return "".join(out).encode()


def read_tagged_gfa(text):
    """-> (segments {name: (letters, LN, RC)} in file order, links [(from, orient, to, orient, overlap, RC)] in file order); every line must be H, S or L, H first."""
    if isinstance(text, bytes):
        text = text.decode()
    lines = text.splitlines()
    assert lines and lines[0] == "H\tVN:Z:1.0" and text.endswith("\n")
    segments, links = {}, []
    for line in lines[1:]:
        f = line.split("\t")
        if f[0] == "S":
            assert not links, "an S line behind an L line"
            assert len(f) == 5 and f[3].startswith("LN:i:") and f[4].startswith("RC:i:") and f[1] not in segments
            segments[f[1]] = (f[2], int(f[3][5:]), int(f[4][5:]))
        else:
            assert f[0] == "L" and len(f) == 7 and f[2] in "+-" and f[4] in "+-" and f[6].startswith("RC:i:"), line
            links.append((f[1], f[2], f[3], f[4], f[5], int(f[6][5:])))
    return segments, links


# ---- the hand-made graph of the device tests and of tests/linkcov_host: six segments (bigraph ids 0/1 .. 10/11), lengths below, at and above the 64 cells a wave takes
# per step; a chain a-b-c-d-e, a side road from b over f's reverse strand to d (links whose canonical form is their mate), and the hairpin e+ -> e-
NAMES = ["a", "b", "c", "d", "e", "f"]
LENGTHS = [1, 63, 64, 65, 130, 7]
GFA_LINKS = [("a", "+", "b", "+"), ("b", "+", "c", "+"), ("c", "+", "d", "+"), ("d", "+", "e", "+"), ("b", "+", "f", "-"), ("f", "-", "d", "+"), ("e", "+", "e", "-")]
HAIRPIN = (8, 9)


def write_graph(path, seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    letters = [bytes(rng.choice(list(b"ACGT"), size=n).tolist()).decode() for n in LENGTHS]
    with open(path, "w") as f:
        for name, s in zip(NAMES, letters):
            f.write(f"S\t{name}\t{s}\n")
        for a, ao, b, bo in GFA_LINKS:
            f.write(f"L\t{a}\t{ao}\t{b}\t{bo}\t0M\n")
    return letters


def graph_links():
    ids = {n: i for i, n in enumerate(NAMES)}
    return sorted({canonical(2 * ids[a] + (ao == "-"), 2 * ids[b] + (bo == "-")) for a, ao, b, bo in GFA_LINKS})


def cases():
    """name -> list of traces (coverage_model.walk over LENGTHS). What each is for stands beside it."""
    from coverage_model import walk
    w = lambda path, start, n, repeats=(): walk(path, start, n, repeats=repeats, lengths=LENGTHS)   # noqa: E731
    return {
        "a traversal at cell 1": [w([0, 2], 0, 10)],                                   # a is one base long
        "a traversal at cell 63": [w([2, 4], 0, 70)],                                  # b's 63 bases, then c in lane 63
        "a traversal at cell 64, over the carry": [w([4, 6], 0, 80)],                  # c's 64 bases fill the first step; lane 0 of the second compares with the carry
        "a traversal at cell 65": [w([6, 8], 0, 100)],                                 # d's 65 bases: lane 1 of the second step
        "one cell": [w([8], 77, 1)],
        "65 cells and no traversal": [w([8], 10, 65)],
        "a traversal right after insertions": [w([2, 4], 50, 40, repeats=set(range(13, 24)))],      # cell 12 is b's last base, cells 13..23 repeat it, cell 24 enters c
        "insertions over the chunk boundary, then a traversal": [w([4, 6], 4, 90, repeats=set(range(60, 70)))],   # cell 59 is c's last base; repeated through lanes 60..63 and 0..5; cell 70 enters d
        "one link on both strands": [w([2, 4], 60, 10), w([5, 3], 60, 10)],            # b+ -> c+ and c- -> b-: one row
        "two alignments share a link": [w([4, 6], 30, 50), w([4, 6, 8], 63, 70)],
        "the hairpin": [w([8, 9], 120, 30)],                                           # e+ to its last base, then e- from its first
        "the side road": [w([2, 11, 6], 60, 20), w([7, 10, 3], 60, 20)],               # b+ f- d+ and its reverse d- f+ b-: canonical forms (2, 11) and (7, 10) both ways
        "the whole chain": [w([0, 2, 4, 6, 8, 9], 0, 400)],
    }


def every_case():
    return [t for traces in cases().values() for t in traces]
