"""Corrected reads, as GraphAligner's sources spell them (the mechanism GraphChainer still carries behind the two option lines it dropped):

  add_corrected       AddCorrected, src/GraphAligner.h:220-231
  get_longest_overlap getLongestOverlap, src/ReadCorrection.cpp:22-36
  get_corrected       getCorrected, src/ReadCorrection.cpp:38-64
  corrected_record / clipped_records   writeCorrectedToQueue / writeCorrectedClippedToQueue, src/Aligner.cpp:313-374

A trace is a list of cells (node, offset, node_switch): bigraph node id, offset in the original node, "the next cell is in another split node". `letter(node, offset)` is
TraceItem::graphCharacter (src/GraphAlignerCommon.h:148-153). Everything is bytes; tolower / toupper are the C locale's, which bytes.lower() / .upper() are."""


def add_corrected(trace, letter):
    assert len(trace) > 0                                                     # :223
    out = bytearray(letter(trace[0][0], trace[0][1]))                         # :225
    for i in range(1, len(trace)):
        prev, cur = trace[i - 1], trace[i]
        if not prev[2] and cur[1] == prev[1] and cur[0] == prev[0]:           # :228
            continue
        out += letter(cur[0], cur[1])                                         # :229
    return bytes(out)


def get_longest_overlap(left, right, max_overlap):
    if len(left) < max_overlap:
        max_overlap = len(left)
    if len(right) < max_overlap:
        max_overlap = len(right)
    for i in range(max_overlap, 0, -1):
        match = True
        for a in range(i):
            if left[len(left) - max_overlap + a] != right[a]:                 # (sic) the window starts max_overlap letters back, whatever i is
                match = False
                break
        if match:
            return i
    return 0


def get_corrected(raw, corrections, max_overlap=0):
    """corrections: (start, end, piece) in the read's output order. max_overlap is getDBGoverlap(): 0 for the 0M graphs this project loads."""
    result = bytearray()
    current_end = 0
    for i, (start, end, piece) in enumerate(corrections):
        assert i == 0 or start >= corrections[i - 1][0]                       # :44
        if start < current_end:
            overlap = get_longest_overlap(bytes(result), piece, max_overlap)
            result += piece[overlap:].upper()
        elif start > current_end:
            result += raw[current_end:start].lower()
            result += piece.upper()
        else:
            result += piece.upper()
        current_end = end                                                     # :60, even when that moves it backwards
    if current_end < len(raw):
        result += raw[current_end:].lower()
    return bytes(result)


def corrected_record(name, raw, corrections, max_overlap=0):
    """One record per read; the id is the whole seq_id. A read without alignments is its lower-cased self (src/Aligner.cpp:984)."""
    return b">" + name + b"\n" + get_corrected(raw, corrections, max_overlap) + b"\n"


def clipped_records(name, corrections):
    """One record per alignment, the piece as AddCorrected left it."""
    return [b">" + name + b"_%d_%d_%d\n" % (i, start, end) + piece + b"\n" for i, (start, end, piece) in enumerate(corrections)]


# ---- over a batch result of graphchainer_amd (keep_traces=True, chain_traces >= 1): what the two files hold for it

def output_order(starts, std_sort=None, sorts=2):
    """The order in which the reference writes alignments whose starts, in the order the selection left them, are `starts`: std::sort by alignmentStart at
    src/Aligner.cpp:1003 and once more at :1023. `std_sort` is libstdc++'s std::sort as a permutation function (tests/stdsort/std_sort_perm.cpp): an insertion sort up to
    16 elements and unstable beyond, so the order of tied starts is defined only by replaying it - and the second sort of an already sorted list may move ties again.
    Without `std_sort` the order is the stable one (what a read with at most 16 alignments gets in any case). Returns indices into `starts`."""
    starts = [int(s) for s in starts]
    if std_sort is None:
        return sorted(range(len(starts)), key=lambda i: starts[i])
    order = list(range(len(starts)))
    for _ in range(sorts):
        order = [order[i] for i in std_sort([starts[i] for i in order])]
    return order


def result_corrections(out, r, letter, std_sort=None):
    """(start, end, piece) of read r's final alignments in output order, from the kept traces: the chained alignment when it won, else the selected whole-read
    alignments sorted by start (src/Aligner.cpp:901-920,1003,1023; output_order). None for a flagged read."""
    if out["failed_assertion"][r] or out["capacity_exceeded"][r]:
        return None
    if out["chained_better"][r]:
        t0, t1 = int(out["read_chain_trace_off"][r]), int(out["read_chain_trace_off"][r + 1])
        trace = list(zip(out["chain_trace_node"][t0:t1].tolist(), out["chain_trace_offset"][t0:t1].tolist(), out["chain_trace_switch"][t0:t1].tolist()))
        return [(int(out["chain_aln_start"][r]), int(out["chain_aln_end"][r]), add_corrected(trace, letter))]
    base = int(out["read_longall_off"][r])
    alns = [base + int(k) for k in out["long_index"][int(out["read_long_off"][r]):int(out["read_long_off"][r + 1])]]
    alns = [alns[i] for i in output_order([out["longall_start"][a] for a in alns], std_sort)]
    got = []
    for a in alns:
        t0, t1 = int(out["long_trace_off"][a]), int(out["long_trace_off"][a + 1])
        trace = list(zip(out["long_trace_node"][t0:t1].tolist(), out["long_trace_offset"][t0:t1].tolist(), out["long_trace_switch"][t0:t1].tolist()))
        got.append((int(out["longall_start"][a]), int(out["longall_end"][a]), add_corrected(trace, letter)))
    return got


def batch_records(out, names, reads, letter, std_sort=None):
    """(records of --corrected-out, records of --corrected-clipped-out) of a batch, in input order."""
    bodies, clipped = [], []
    for r, (name, raw) in enumerate(zip(names, reads)):
        corrections = result_corrections(out, r, letter, std_sort)
        if corrections is None:
            continue
        bodies.append(corrected_record(name, raw, corrections))
        clipped += clipped_records(name, corrections)
    return bodies, clipped
