"""Coverage of the graph by the alignments a run writes (--coverage-out / --base-coverage-out; include/graphchainer_amd.h has the definition), stated twice in plain
Python and held to each other by test_coverage_model.py:

  from_traces   the per-cell rule over traces in output coordinates (bigraph node id, offset in the original node): cell i covers the base under it iff i == 0 or its
                (node, offset) differs from cell i-1's; the base is on segment node // 2 at `offset` for an even id, at length - 1 - offset for an odd one
  from_vg_json  the mapping intervals of the vg JSON the same run writes: every mapping covers [position.offset, position.offset + sum of from_length) of its node in
                its orientation

Both return one int64 depth array per segment; bases[segment] is its sum. segment_table / base_table are the two file writers."""
import json

import numpy as np


def read_gfa_segments(path):
    """-> (names, lengths) in internal segment order: the order in which the GFA first names a segment, in an S line or in an L line."""
    index, lengths = {}, {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            index.setdefault(f[1], len(index))
            lengths[f[1]] = len(f[2])
        elif f[0] == "L":
            index.setdefault(f[1], len(index))
            index.setdefault(f[3], len(index))
    names = sorted(index, key=index.get)
    return names, [lengths[n] for n in names]


def from_traces(node, offset, trace_off, segment_length):
    depth = [np.zeros(int(n), dtype=np.int64) for n in segment_length]
    for a in range(len(trace_off) - 1):
        b, e = int(trace_off[a]), int(trace_off[a + 1])
        for i in range(b, e):
            if i == b or int(node[i]) != int(node[i - 1]) or int(offset[i]) != int(offset[i - 1]):
                seg, length = int(node[i]) // 2, int(segment_length[int(node[i]) // 2])
                assert 0 <= int(offset[i]) < length
                depth[seg][int(offset[i]) if int(node[i]) % 2 == 0 else length - 1 - int(offset[i])] += 1
    return depth


def from_vg_json(lines, segment_ids, segment_length):
    """lines: vg::Alignment documents (JSON text or dicts); segment_ids: {segment name: internal segment number} (Position.name; a node_id of 0 is not printed)."""
    depth = [np.zeros(int(n), dtype=np.int64) for n in segment_length]
    for line in lines:
        doc = json.loads(line) if isinstance(line, (str, bytes)) else line
        for mapping in doc.get("path", {}).get("mapping", []):
            pos = mapping["position"]
            seg = segment_ids[pos["name"]]
            assert int(pos.get("node_id", 0)) == seg
            length = int(segment_length[seg])
            start = int(pos.get("offset", 0))
            end = start + sum(int(e.get("from_length", 0)) for e in mapping.get("edit", []))
            assert 0 <= start <= end <= length
            if pos.get("is_reverse", False):
                start, end = length - end, length - start
            depth[seg][start:end] += 1
    return depth


def bases_of(depth):
    return np.array([int(d.sum()) for d in depth], dtype=np.uint64)


def flat(depth):
    return np.concatenate([np.zeros(0, dtype=np.int64)] + list(depth))


def shown(name, index):
    return str(name) if str(name) != "" else str(index)


def segment_table(names, depth):
    out = ["#segment\tlength\tbases\n"]
    for i, (name, d) in enumerate(zip(names, depth)):
        out.append(f"{shown(name, i)}\t{len(d)}\t{int(d.sum())}\n")
    return "".join(out).encode()


def base_table(names, depth):
    out = []
    for i, (name, d) in enumerate(zip(names, depth)):
        start = 0
        while start < len(d):
            end = start + 1
            while end < len(d) and d[end] == d[start]:
                end += 1
            if d[start] != 0:
                out.append(f"{shown(name, i)}\t{start}\t{end}\t{int(d[start])}\n")
            start = end
    return "".join(out).encode()


# ---- the exact shapes the host program (tests/coverage_host) and the device tests walk: four segments of 1, 64, 65 and 130 bp (bigraph ids 0/1 .. 6/7; the last one
# is three split nodes of the aligner's graph), traces of 1, 63, 64, 65 and 129 cells - below, at and above the 64 cells a wave takes per step
SHAPE_LENGTHS = [1, 64, 65, 130]


def walk(path, start, n, repeats=(), lengths=SHAPE_LENGTHS):
    """A trace of n cells along the bigraph nodes of `path` from offset `start` of the first: a cell whose index is in `repeats` stands where the one before it does (an
    insertion), every other one advances by a base, into the next node of the path behind a node's last base. -> (nodes, offsets)"""
    nodes, offsets, k, offset = [], [], 0, start
    for i in range(n):
        if i > 0 and i not in repeats:
            offset += 1
            if offset == lengths[path[k] // 2]:
                k, offset = k + 1, 0
        nodes.append(path[k])
        offsets.append(offset)
    return nodes, offsets


def shape_cases():
    """name -> list of traces. Between them: every trace length, an insertion run across a chunk boundary and one in lanes 0 and 63, both strands of s4, depths 2 and 3
    from repeated traces, equal depth on both sides of a segment boundary, a depth change on a segment's last base, runs of segments changing inside a chunk."""
    forward, backward = [0, 2, 4, 6], [7, 5, 3, 1]
    return {
        "one cell": [walk([6], 77, 1)],
        "63 cells": [walk([6], 0, 63)],
        "64 cells to the segment's last base": [walk([6], 66, 64)],
        "65 cells, a whole segment": [walk([4], 0, 65)],
        "129 cells over three segments": [walk(forward, 0, 129)],                                   # s1, s2 and s3[0:64) at one depth: the runs still end at the boundaries
        "insertions across the chunk boundary": [walk([6], 0, 129, repeats=set(range(60, 69)))],
        "insertions in lanes 0 and 63": [walk([6], 3, 129, repeats={63, 64, 127, 128})],
        "an insertion run at the start": [walk([2], 10, 65, repeats=set(range(1, 20)))],
        "the reverse strand": [walk(backward, 100, 129)],                                             # s4[0:30) backwards, s3 whole, s2[30:64)
        "both strands of s4": [walk([6], 20, 64), walk([7], 20, 64)],                                # forward [20, 84) and [46, 110)
        "depth three": [walk([4], 30, 35)] * 3,                                                       # s3[30:65) three times: the change from 0 falls inside, the end on the last base
        "the last base alone": [walk([4], 64, 1), walk([0], 0, 1), walk([1], 0, 1)],
        "segments changing inside a chunk": [walk([0, 2], 0, 40), walk([5, 3, 1], 60, 70)],
    }


def shape_sets():
    """name -> list of traces, as the handles of the tests are filled."""
    cases = shape_cases()
    everything = [t for traces in cases.values() for t in traces]
    return {"every case": everything,
            "s1 stays uncovered": cases["63 cells"] + cases["65 cells, a whole segment"] + cases["depth three"] + cases["both strands of s4"],
            **{name: traces for name, traces in cases.items()}}


def traces_depth(traces, lengths=SHAPE_LENGTHS):
    node = [n for t in traces for n in t[0]]
    offset = [o for t in traces for o in t[1]]
    off = np.concatenate([[0], np.cumsum([len(t[0]) for t in traces])]).astype(np.int64)
    return from_traces(node, offset, off, lengths)
