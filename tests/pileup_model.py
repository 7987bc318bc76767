"""The pileup of the alignments a run writes (--pileup-out; include/graphchainer_amd.h has the definition), stated twice in plain Python and held to each other by
test_pileup_model.py:

  from_cells    the per-cell rule over one trace in output coordinates with the read positions of its cells: with `covers` = (i == 0 or (node, offset) differs from cell
                i-1's) and `moved` = (i == 0 or seqPos differs), covers and moved is an aligned pair (a mismatch when the IUPAC sets of read and graph letter do not
                meet), covers alone a deletion, moved alone an insertion, neither nothing
  from_vg_json  the edits of the vg JSON the same run writes, mapping by mapping: kinds and lengths from from_length / to_length, a mismatch where an edit with both
                lengths carries `sequence`, the read letters from the document's own sequence at the position the edits have advanced to

Both fill a Pileup: per segment a depth array and rows [length, 8] in the order of CHANNELS, forward coordinates. table() is the file writer with its filter."""
import json

import numpy as np

import coverage_model as cm

CHANNELS = ("mmA", "mmC", "mmG", "mmT", "mmN", "del", "ins_after", "ins_before")
MM_N, DEL, INS_AFTER, INS_BEFORE = 4, 5, 6, 7
HEAD = "#segment\tpos\tref\tdepth\tmatch\tmmA\tmmC\tmmG\tmmT\tmmN\tdel\tins_before\tins_after\n"

# sets of plain bases: A 1, C 2, G 4, T 8; a byte that is no nucleotide code has the empty set and matches nothing
IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "K": 12, "M": 3, "S": 6, "W": 9, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
LETTER_OF_SET = "NACMGRSVTWYHKDBN"


def letter_set(letter):
    return IUPAC.get(letter.upper(), 0)


def complement_set(s):
    return (s & 1) << 3 | (s & 2) << 1 | (s & 4) >> 1 | (s & 8) >> 3


def read_channel(letter, odd):
    """The mismatch channel of a read letter: A C G T/U (either case) their own, anything else mmN; complemented on an odd node id."""
    k = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(letter.upper(), MM_N)
    return 3 - k if odd and k < MM_N else k


class Segments:
    """names and forward letters in internal segment order (coverage_model.read_gfa_segments's order)."""

    def __init__(self, names, letters):
        self.names, self.letters = list(names), list(letters)
        self.lengths = [len(x) for x in self.letters]
        self.ids = {n: i for i, n in enumerate(self.names)}

    @classmethod
    def from_gfa(cls, path):
        names, _ = cm.read_gfa_segments(path)
        letters = {}
        for line in open(path):
            f = line.rstrip("\n").split("\t")
            if f[0] == "S":
                letters[f[1]] = f[2]
        return cls(names, [letters[n] for n in names])

    def graph_set(self, node, offset):
        """The set of the letter under (bigraph node, offset): the forward letter for an even id, the complement of the one at length - 1 - offset for an odd one."""
        seg = node // 2
        if node % 2 == 0:
            return letter_set(self.letters[seg][offset]) or 15
        return complement_set(letter_set(self.letters[seg][self.lengths[seg] - 1 - offset]) or 15)


class Pileup:
    def __init__(self, segments):
        self.segments = segments
        self.depth = [np.zeros(n, dtype=np.int64) for n in segments.lengths]
        self.rows = [np.zeros((n, 8), dtype=np.int64) for n in segments.lengths]

    def add(self, other):
        for k in range(len(self.depth)):
            self.depth[k] += other.depth[k]
            self.rows[k] += other.rows[k]
        return self

    def flat_rows(self):
        return np.concatenate([np.zeros((0, 8), dtype=np.int64)] + self.rows)

    def flat_depth(self):
        return cm.flat(self.depth)

    def totals(self):
        return {c: int(self.flat_rows()[:, k].sum()) for k, c in enumerate(CHANNELS)}


def from_cells(node, offset, seq_pos, read, segments, into=None):
    """One trace. read: the read's letters (str or bytes)."""
    read = read.decode("latin-1") if isinstance(read, (bytes, bytearray)) else read
    p = into if into is not None else Pileup(segments)
    for i in range(len(node)):
        n, o, q = int(node[i]), int(offset[i]), int(seq_pos[i])
        covers = i == 0 or n != int(node[i - 1]) or o != int(offset[i - 1])
        moved = i == 0 or q != int(seq_pos[i - 1])
        seg, odd = n // 2, n % 2 == 1
        length = segments.lengths[seg]
        assert 0 <= o < length and 0 <= q < len(read)
        at = length - 1 - o if odd else o
        if covers:
            p.depth[seg][at] += 1
        if covers and moved:
            if not letter_set(read[q]) & segments.graph_set(n, o):
                p.rows[seg][at][read_channel(read[q], odd)] += 1
        elif covers:
            p.rows[seg][at][DEL] += 1
        elif moved:
            p.rows[seg][at][INS_BEFORE if odd else INS_AFTER] += 1
    return p


def from_traces(traces, seq_pos, reads, segments):
    p = Pileup(segments)
    for (node, offset), q, read in zip(traces, seq_pos, reads):
        from_cells(node, offset, q, read, segments, into=p)
    return p


def from_vg_json(doc, segments, into=None):
    """One vg::Alignment document (JSON text or dict). The read letters are the document's sequence at the position the edits have advanced to - not the edit's own
    sequence field, whose first letter is the read's first whatever the alignment's start. An insertion counts into the base before the mapping's current offset in walk
    direction; as a mapping's first edit, into the previous mapping's last base."""
    doc = json.loads(doc) if isinstance(doc, (str, bytes)) else doc
    p = into if into is not None else Pileup(segments)
    read, q, last = doc.get("sequence", ""), 0, None      # last: (segment, forward position, reverse) of the base the walk stood on last
    for mapping in doc.get("path", {}).get("mapping", []):
        pos = mapping["position"]
        seg, reverse = segments.ids[pos["name"]], bool(pos.get("is_reverse", False))
        length, cur = segments.lengths[seg], int(pos.get("offset", 0))
        fwd = (lambda x: length - 1 - x) if reverse else (lambda x: x)      # noqa: E731
        for edit in mapping.get("edit", []):
            fl, tl = int(edit.get("from_length", 0)), int(edit.get("to_length", 0))
            if fl and tl:
                assert fl == tl
                for k in range(fl):
                    at = fwd(cur + k)
                    p.depth[seg][at] += 1
                    if "sequence" in edit:
                        p.rows[seg][at][read_channel(read[q + k], reverse)] += 1
                    last = (seg, at, reverse)
                cur, q = cur + fl, q + tl
            elif fl:
                for k in range(fl):
                    at = fwd(cur + k)
                    p.depth[seg][at] += 1
                    p.rows[seg][at][DEL] += 1
                    last = (seg, at, reverse)
                cur += fl
            elif tl:
                assert last is not None, "an alignment does not begin with an insertion: its first cell stands on a base"
                s, at, rev = last
                p.rows[s][at][INS_BEFORE if rev else INS_AFTER] += tl
                q += tl
        assert 0 <= cur <= length
    return p


def passes(depth, row, min_alt, min_fraction):
    alt = int(max(row))
    return depth > 0 and alt >= min_alt and float(alt) >= min_fraction * float(depth)


def table(p, first=0, count=None, min_alt=1, min_fraction=0.0):
    """The file: the head line when first == 0, then a line per passing base of forward bases [first, first + count) in the order of the depth array."""
    segments = p.segments
    out = [HEAD] if first == 0 else []
    i, end = 0, None if count is None else first + count
    for s, name in enumerate(segments.names):
        for at in range(segments.lengths[s]):
            if i >= first and (end is None or i < end):
                d, row = int(p.depth[s][at]), [int(v) for v in p.rows[s][at]]
                if passes(d, row, min_alt, min_fraction):
                    ref = LETTER_OF_SET[letter_set(segments.letters[s][at])]
                    match = d - sum(row[:DEL + 1])
                    out.append("\t".join([cm.shown(name, s), str(at), ref, str(d), str(match)] + [str(v) for v in row[:DEL + 1]] + [str(row[INS_BEFORE]), str(row[INS_AFTER])]) + "\n")
            i += 1
    return "".join(out).encode()


# ---- the exact shapes the host program (tests/pileup_host) and the device tests walk: coverage_model's four segments with letters of their own, traces of 1, 63, 64, 65
# and 129 cells with read positions and reads
SHAPE_NAMES = ["s1", "s2", "s3", "s4"]
SHAPE_LENGTHS = cm.SHAPE_LENGTHS


def shape_letters():
    rng = np.random.default_rng(5)
    letters = ["".join(rng.choice(list("ACGT"), size=n).tolist()) for n in SHAPE_LENGTHS]
    s3 = list(letters[2])
    s3[10], s3[11], s3[40] = "R", "N", "Y"          # ambiguous graph letters: the split node is one of the aligner's ambiguous ones
    letters[2] = "".join(s3)
    return letters


def shape_segments():
    return Segments(SHAPE_NAMES, shape_letters())


COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "N": "N"}


def walk(segments, path, start, n, ins=(), dels=(), same=(), wrong=None):
    """A trace of n cells along the bigraph nodes of `path` from offset `start` of the first, with its read. Cell i > 0 in `ins` stands where the cell before does and takes
    the next read base; in `dels` it advances in the graph on the same read base; in `same` it repeats the cell before altogether; every other cell advances in both.
    wrong: {cell index: read letter} replaces the read letter under that cell (otherwise a letter of the graph letter's set, so a match). -> ((nodes, offsets), seq_pos, read)"""
    wrong = wrong or {}
    nodes, offsets, seq_pos, read, k, offset, q = [], [], [], [], 0, start, 0
    for i in range(n):
        if i > 0 and i not in same:
            if i not in ins:
                offset += 1
                if offset == segments.lengths[path[k] // 2]:
                    k, offset = k + 1, 0
            if i not in dels:
                q += 1
        nodes.append(path[k])
        offsets.append(offset)
        seq_pos.append(q)
        if q == len(read):
            graph = LETTER_OF_SET[segments.graph_set(path[k], offset)]
            letter = {"R": "G", "Y": "C", "N": "T"}.get(graph, graph)
            read.append(wrong.get(i, letter if i not in ins else "ACGT"[i % 4]))
    return (nodes, offsets), seq_pos, "".join(read).encode()


def shape_cases(segments=None):
    """name -> list of (trace, seq_pos, read). Between them: every trace length; a mismatch in lanes 0 and 63; a deletion run and an insertion run each across the 64-cell
    chunk boundary; both strands of s4; one base under three traces; every mismatch channel on both strands, lower case, U and N in the read; ambiguous graph letters that
    the read letter matches and does not; a cell that repeats the one before altogether."""
    g = segments or shape_segments()
    forward, backward = [0, 2, 4, 6], [7, 5, 3, 1]

    def other(node, offset, shift=1):          # a plain letter that is not under (node, offset)
        have = g.graph_set(node, offset)
        return [x for x in "ACGT"[shift:] + "ACGT"[:shift] if not letter_set(x) & have][0]
    return {
        "one cell, a mismatch": [walk(g, [6], 77, 1, wrong={0: other(6, 77)})],
        "63 cells": [walk(g, [6], 0, 63, wrong={62: other(6, 62)})],
        "64 cells, mismatches in lanes 0 and 63": [walk(g, [6], 66, 64, wrong={0: other(6, 66), 63: other(6, 129)})],
        "65 cells, a whole segment with ambiguous letters": [walk(g, [4], 0, 65, wrong={10: "C", 11: "a", 40: "t", 64: other(4, 64, 2)})],      # R does not hold C; N holds a; Y holds t
        "129 cells over three segments": [walk(g, forward, 0, 129, wrong={0: other(0, 0), 63: other(2, 62), 64: other(2, 63), 127: other(4, 62), 128: "N"})],
        "deletions across the chunk boundary": [walk(g, [6], 0, 129, dels=set(range(60, 69)))],
        "insertions across the chunk boundary": [walk(g, [6], 0, 129, ins=set(range(60, 69)))],
        "insertions and deletions in lanes 0 and 63": [walk(g, [6], 3, 129, ins={63, 64}, dels={127, 128})],
        "an insertion run at the start": [walk(g, [2], 10, 65, ins=set(range(1, 20)))],
        "a deletion across a node change": [walk(g, [2, 4], 60, 12, dels={3, 4, 5})],
        "the reverse strand": [walk(g, backward, 100, 129, ins={5, 70}, dels={9, 64}, wrong={0: "a", 1: "c", 2: "g", 3: "u", 30: "N", 63: "x"})],
        "both strands of s4": [walk(g, [6], 20, 64, wrong={30: other(6, 50)}), walk(g, [7], 20, 64, wrong={30: other(7, 50)}, ins={40})],
        "three traces over one base": [walk(g, [4], 30, 35, wrong={5: other(4, 35)}), walk(g, [4], 30, 35, wrong={5: other(4, 35, 2)}), walk(g, [5], 0, 35, dels={29})],
        "cells that repeat altogether": [walk(g, [6], 5, 70, same={3, 63, 64, 65}, ins={10})],
        "every channel, lower case and U": [walk(g, [2], 0, 64, wrong={i: x for i, x in enumerate("acgtuACGTUnN-")}), walk(g, [3], 0, 64, wrong={i: x for i, x in enumerate("acgtuACGTUnN-")})],
    }


def shape_sets():
    cases = shape_cases()
    everything = [t for traces in cases.values() for t in traces]
    return {"every case": everything, **cases}


def shape_pileup(items, segments=None):
    g = segments or shape_segments()
    return from_traces([t for t, _, _ in items], [q for _, q, _ in items], [r for _, _, r in items], g)
