"""The chained alignment of --fast-mode, restated from the reference (src/Aligner.cpp:409-424,834-843,880-895): the trace is the stitched piece itself,
one cell per path base, cell j at read position min(y, x + j); the score counts the cells whose graph letter is not the read's letter there."""


def path_to_trace(path, first_offset, last_offset, node_length):
    """pathToTrace (:409-424): (split node, offset) of every base of the piece. Nodes are compared by value, so a one-node piece takes the first branch alone
    and runs from first_offset to the node's END, not to last_offset."""
    cells = []
    for node in path:
        s, l = 0, node_length[node]
        if node == path[0]:
            s = first_offset
        elif node == path[-1]:
            l = last_offset + 1
        cells.extend((node, o) for o in range(s, l))
    return cells


def fast_chained_alignment(path, first_offset, last_offset, x, y, read, node_length, node_ids, node_offset, letter):
    """path: the split nodes of `longest`; (x, y): A[ids[0]].x and A[ids.back()].y of the read's CHAIN (:836); letter(split node, offset) -> the graph's character.
    Returns (trace_node, trace_offset, trace_seqpos, trace_switch, score, aln_start, aln_end) in output coordinates (:880-887: bigraph node id, offset in the
    original node, "the next cell lies in another split node"); aln_start / aln_end are None for an empty piece (no alignment item, :890)."""
    longest = path_to_trace(path, first_offset, last_offset, node_length)
    read = bytes(read) if not isinstance(read, str) else read.encode()
    seqpos, score = [], 0
    for j, (node, o) in enumerate(longest):
        p = min(y, x + j)                                              # :838
        seqpos.append(p)
        if ord(letter(node, o)) != read[p]:                            # :839-840, chars as they are
            score += 1
    trace_node = [node_ids[node] for node, _ in longest]               # :886-887
    trace_offset = [o + node_offset[node] for node, o in longest]
    trace_switch = [1 if j + 1 < len(longest) and longest[j][0] != longest[j + 1][0] else 0 for j in range(len(longest))]   # :880-883
    if not longest:
        return [], [], [], [], score, None, None
    return trace_node, trace_offset, seqpos, trace_switch, score, seqpos[0], seqpos[-1] + 1                                   # :893-895
