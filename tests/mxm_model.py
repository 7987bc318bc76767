"""Brute-force model of the MUM / MEM seeder (gc_seeds_mxm; the reference's MummerSeeder, src/MummerSeeder.cpp), written from the definitions alone - no suffix array:

  text      every segment forward, in ascending node id, each followed by a separator; a c g t (u) in either case are letters, anything else is a separator (lowercaseRef)
  read      the same letters, anything else is 'x' and equals nothing (lowercaseSeq); the reverse strand is the reverse complement, 'x' stays 'x'
  MEM       (p, i, l): l >= min_len, T[p:p+l] == q[i:i+l] over a c g t, i == 0 or p == 0 or T[p-1] != q[i-1], and the same at p+l, i+l - by direct extension from a
            dictionary of the text's min_len-mers
  MUM       mummer's MAM: a MEM whose matched string occurs exactly once in the text (counted, overlapping occurrences included)
  reverse   a match (p, i, l) of the reverse strand: nodeOffset = nodeLen - off - l, seqPos = readLen - i - l, reverse = 1 (matchesToSeeds)
  order     matchLen descending, forward before reverse, query position in the searched orientation, text position; the first `count` are kept. This order is the library's
            own: the reference's follows mummer's emission order through a priority queue and an unstable sort and cannot be reproduced without mummer.
A hit is (node_id, node_offset, seq_pos, match_len, raw_goodness = match_len, reverse)."""
import bisect

_REF = bytearray(b"$" * 256)
_READ = bytearray(b"x" * 256)
for _letters, _to in ((b"Aa", b"a"), (b"Cc", b"c"), (b"Gg", b"g"), (b"TtUu", b"t")):
    for _c in _letters:
        _REF[_c] = _to[0]
        _READ[_c] = _to[0]
_REF, _READ = bytes(_REF), bytes(_READ)
_COMPLEMENT = bytes.maketrans(b"acgt", b"tgca")
_IUPAC = set(b"ACGTURYKMSWBDHVNacgturykmswbdhvn")

MUM, MEM = 1, 2


def map_ref(seq):
    return bytes(seq).translate(_REF)


def map_read(seq):
    return bytes(seq).translate(_READ)


def reverse_strand(mapped):
    return mapped.translate(_COMPLEMENT)[::-1]


def read_is_flagged(read):
    """A letter outside the IUPAC alphabet: the batch flags the read at upload and no stage touches it."""
    return any(c not in _IUPAC for c in bytes(read))


def gfa_segments(path):
    """{node id: sequence} of a GFA. A segment's node id is the rank of its name's first appearance on an S or L line (getNameId, src/GfaGraph.cpp:146-156), whatever the name."""
    ids, out = {}, {}
    for line in open(path):
        f = line.split()
        if f and f[0] == "S":
            out[ids.setdefault(f[1], len(ids))] = f[2].encode()
        elif f and f[0] == "L":
            ids.setdefault(f[1], len(ids))
            ids.setdefault(f[3], len(ids))
    return out


class Text:
    def __init__(self, segments):
        """segments: {node id: sequence (bytes or str)}"""
        self.ids = sorted(segments)
        self.starts = []
        parts = []
        at = 0
        for i in self.ids:
            s = segments[i]
            s = s.encode() if isinstance(s, str) else bytes(s)
            self.starts.append(at)
            parts.append(map_ref(s) + b"$")
            at += len(s) + 1
        self.starts.append(at)
        self.T = b"".join(parts)
        self._kmers = {}
        self._once = {}

    def kmers(self, k):
        if k not in self._kmers:
            d = {}
            T = self.T
            for p in range(len(T) - k + 1):
                w = T[p:p + k]
                if b"$" not in w:
                    d.setdefault(w, []).append(p)
            self._kmers[k] = d
        return self._kmers[k]

    def occurs_once(self, s):
        if s not in self._once:
            first = self.T.find(s)
            self._once[s] = first >= 0 and self.T.find(s, first + 1) < 0
        return self._once[s]

    def locate(self, p):
        """text position -> (node id, offset in the segment, the segment's length)"""
        k = bisect.bisect_right(self.starts, p) - 1
        return self.ids[k], p - self.starts[k], self.starts[k + 1] - self.starts[k] - 1


def _common(a, i, b, j):
    """length of the common prefix of a[i:] and b[j:]"""
    n = 0
    while True:
        x, y = a[i + n:i + n + 64], b[j + n:j + n + 64]
        if x and x == y:
            n += len(x)
            if len(x) < 64:
                return n
            continue
        m = min(len(x), len(y))
        k = 0
        while k < m and x[k] == y[k]:
            k += 1
        return n + k


def mems(text, q, min_len):
    """MEMs of one mapped strand q: [(p, i, l)], plus the largest number of occurrences of one window"""
    T = text.T
    table = text.kmers(min_len)
    out = []
    widest = 0
    for i in range(len(q) - min_len + 1):
        occ = table.get(q[i:i + min_len])
        if not occ:
            continue
        widest = max(widest, len(occ))
        for p in occ:
            if i > 0 and p > 0 and T[p - 1] == q[i - 1]:
                continue
            out.append((p, i, min_len + _common(T, p + min_len, q, i + min_len)))
    return out, widest


def matches(text, read, mode, min_len, stats=None):
    """The read's matches over both strands in the defined order: [(l, strand, i, p)]"""
    out = []
    fw = map_read(read)
    for strand, q in ((0, fw), (1, reverse_strand(fw))):
        found, widest = mems(text, q, min_len)
        if stats is not None:
            stats["widest"] = max(stats.get("widest", 0), widest)
        for p, i, l in found:
            if mode == MEM or text.occurs_once(q[i:i + l]):
                out.append((l, strand, i, p))
    out.sort(key=lambda m: (-m[0], m[1], m[2], m[3]))
    return out


def seeds(text, read, mode, min_len=20, count=None, stats=None):
    """What MxmIndex.seeds(...).hits() holds for the read: the first `count` (None or -1: all) of the defined order, as hits"""
    assert min_len >= 2 and mode in (MUM, MEM)
    if read_is_flagged(read):
        return []
    found = matches(text, read, mode, min_len, stats)
    if count is not None and count != -1:
        found = found[:count]
    hits = []
    for l, strand, i, p in found:
        node, off, node_len = text.locate(p)
        if strand:
            hits.append((node, node_len - off - l, len(read) - i - l, l, l, 1))
        else:
            hits.append((node, off, i, l, l, 0))
    return hits
