"""The inputs of tests/test_letters_model.py and tests/test_letters_gpu.py: the graph of the extension modes' GPU tests (SynthGraph(40_000, seed=23, repeats=3)) with
IUPAC codes, lower case and U written into its segments, and reads of those tests' shapes cut from windows that cross the rewritten segments, plus reads that carry
the letters themselves. Everything follows from fixed seeds. LettersInputs keeps the models' results per setting, as ClipInputs does."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeding_model                                                     # noqa: E402
from alignment_model import AlignmentModel, reverse_complement           # noqa: E402
from extension_model import ModelAssertion                               # noqa: E402
from test_precise_clipping_gpu import ClipInputs                         # noqa: E402

CODES = "NRYKMSWBDHV"
SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "N": "ACGT", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
# backbone windows whose segments stay as they are: the lockstep fragment kernel declines an extension that touches an ambiguous node, so it needs stretches
# without one to accept work on; and the one-slice reads have few minimizers to lose
UNTOUCHED = {
    "fragment kernel": (5000, 5700),
    "half of the patchy fragments": (22300, 22700),
    "the 50-base read": (16990, 17060),
}


def _code_for(rng, base, contains):
    """An IUPAC code whose set holds `base`, or one whose set does not (N has no such base)."""
    return rng.choice([c for c in CODES if (base in SETS[c]) == contains])


def rewrite_gfa(sg, source, target, iupac=True):
    """`source` is sg.write_gfa's file. One IUPAC code in every third backbone segment of 12 bases or more, outside UNTOUCHED: two in three hold the base they
    replace. Every fifth backbone segment in lower case, every seventh with U for T (the graph build folds both). Returns {backbone position: (base, code)}.
    iupac=False leaves the codes out and keeps the rest: the graph on which the tests' coverage assertions must fail."""
    rng = random.Random(7)
    n = len(sg.seg_start)
    # segment i is the (i + #nodes of the sites before it)-th S line: a SNP site adds two allele nodes, an insertion one
    line_of = np.arange(n) + np.concatenate([[0], np.cumsum(np.where(sg.is_snp, 2, 1))])
    segment_of_line = {int(l): i for i, l in enumerate(line_of)}
    placed, out, s_line, eligible = {}, [], 0, 0
    for line in open(source, "rb"):
        if line.startswith(b"S\t"):
            f = line.rstrip(b"\n").split(b"\t")
            i = segment_of_line.get(s_line)
            s_line += 1
            if i is not None:
                a, b = int(sg.seg_start[i]), int(sg.seg_end[i])
                seq = bytearray(f[2])
                assert len(seq) == b - a
                if b - a >= 12 and not any(a < hi and lo < b for lo, hi in UNTOUCHED.values()):
                    eligible += 1
                    if eligible % 3 == 0:
                        at = rng.randrange(b - a)
                        base = chr(seq[at])
                        code = CODES[(eligible // 3) % len(CODES)]
                        contains = (eligible // 3) % 3 != 2
                        if (base in SETS[code]) != contains:                 # keep the round-robin over the codes where it fits, else draw one that does
                            code = _code_for(rng, base, contains)
                        if iupac:
                            seq[at] = ord(code)
                            placed[a + at] = (base, code)
                if i % 5 == 2:
                    seq = bytearray(bytes(seq).lower())
                if i % 7 == 3:
                    seq = bytearray(bytes(seq).replace(b"T", b"U").replace(b"t", b"u"))
                f[2] = bytes(seq)
                line = b"\t".join(f) + b"\n"
        out.append(line)
    with open(target, "wb") as f:
        f.writelines(out)
    return placed


class LettersInputs(ClipInputs):
    """ClipInputs on the rewritten graph. `whole`: the whole-read pass's reads; `fragments`: the 64-base fragment reads; `iupac_reads`, `lowercase_reads`: indices
    into `whole` of the reads that carry codes / lower case; `no_seed_reads`: of those that must come back empty."""

    def __init__(self, directory, iupac=True):
        super().__init__(directory)
        plain = self.gfa
        self.gfa = os.path.join(str(directory), "letters.gfa")
        self.placed = rewrite_gfa(self.sg, plain, self.gfa, iupac)
        sg, bb = self.sg, self.bb
        rng = random.Random(5)

        def rnd(n):
            return bytes(rng.choice(b"ACGT") for _ in range(n))

        def anti(a, n):      # (as Inputs: letters that match the backbone on none of the near diagonals)
            out = bytearray()
            for i in range(a, a + n):
                near, wide = set(bb[i - 1:i + 2]), set(bb[i - 2:i + 3])
                out.append(([c for c in b"ACGT" if c not in wide] or [c for c in b"ACGT" if c not in near] or [bb[i] ^ 6])[0])
            return bytes(out)

        def patchy(a, n, exact, w, junk):
            return b"".join(bb[l:l + exact] + junk(l + exact, w - exact) for l in range(a, a + n, w))

        def with_codes(a, n, every, contains):
            """backbone[a:a+n] with an IUPAC code at every `every`-th base, each holding the base it replaces - or not."""
            s = bytearray(bb[a:a + n])
            for k, i in enumerate(range(every // 2, n, every)):
                code = CODES[k % len(CODES)]
                if (chr(s[i]) in SETS[code]) != contains:
                    code = _code_for(rng, chr(s[i]), contains)
                s[i] = ord(code)
            return bytes(s)

        n_run = bytearray(bb[8000:8400])
        n_run[180:220] = b"N" * 40
        hand_built = [
            bytes(n_run),                                                      # a 40-base run of N
            bb[11000:11350].lower(),                                           # lower case
            with_codes(18000, 430, 71, True),                                  # a code every 71 bases, each holding its base: the seeds between them survive
            with_codes(18000, 430, 71, True).lower(),
            with_codes(24000, 430, 71, False),                                 # codes that do not hold the base: mismatches
            bb[27000:27300].replace(b"T", b"U"),                               # U for T: no minimizer matches, so no seed - empty, not failed
        ]
        self.whole = sg.sample_reads(3, 700, seed=9, p_del=0.07, p_sub=0.08, p_ins=0.07) + [
            bb[4000:4500] + bb[20000:20500],                                   # a chimera
            bb[30000:30300] + rnd(600),                                        # junk tail, head, middle
            rnd(500) + bb[10000:10200],
            bb[12000:12200] + rnd(300) + bb[12500:12700],
            patchy(22000, 700, 17, 35, lambda a, n: rnd(n)),
            bb[26000:26200] + patchy(26200, 350, 17, 35, lambda a, n: rnd(n)),
            bb[15000:15064],                                                   # exactly one slice
            bb[16000:16128],                                                   # exactly two
            bb[17000:17050],                                                   # one partial slice
        ] + self._extra() + hand_built + [reverse_complement(r) for r in hand_built]
        first = len(self.whole) - 2 * len(hand_built)
        self.hand_built = list(range(first, len(self.whole)))
        self.iupac_reads = [first + k for k in (0, 2, 3, 4)] + [first + len(hand_built) + k for k in (0, 2, 3, 4)]
        self.lowercase_reads = [first + 1, first + 3, first + len(hand_built) + 1, first + len(hand_built) + 3]
        self.no_seed_reads = [first + 5]
        self.fragments = [
            patchy(22000, 640, 20, 64, anti),
            patchy(5000, 640, 24, 64, anti),
            rnd(3) + patchy(9000, 640, 18, 64, anti),
            patchy(30000, 320, 22, 64, anti) + bb[30320:30640],
        ]
        self._runs = {}

    def _extra(self):
        from test_precise_model import _extra_reads
        return _extra_reads(self)

    def graph(self):
        """extension_model.Graph of the rewritten GFA."""
        return self.world()[2]

    def ambiguous(self):
        """Per split node: does it hold a letter outside ACGT."""
        if not hasattr(self, "_ambiguous"):
            self._ambiguous = [any(c not in "ACGT" for c in s) for s in self.graph().sequence]
        return self._ambiguous

    def seeds(self, std_sort, read):
        graph, index, _, _ = self.world()
        return seeding_model.order_seeds_by_chaining(seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort), graph, std_sort)

    def run(self, std_sort, cls, which, whole_read, bandwidth=10, split=35, **band):
        """(per read (whole-read alignments, anchors) or None where the model trips one of the reference's assertions, the extension model); once per setting."""
        key = (cls.__name__, which, whole_read, bandwidth, split, tuple(sorted(band.items())))
        if key not in self._runs:
            _, _, g, original_size = self.world()
            ext = cls(g, bandwidth, **band)
            model = AlignmentModel(ext, g, original_size)
            out = []
            for read in getattr(self, which):
                seeds = self.seeds(std_sort, read)
                try:
                    alns = []
                    if whole_read and seeds:
                        got, _ = model.align_one_way(read, seeds, True)
                        alns = [(a["start"], a["end"], a["score"], [tuple(c) for c in a["trace"]]) for a in got]
                    anchors = [(x, y, score, list(path)) for (x, y, path, first, last, score)
                               in model.anchors_of_read(read, seeding_model.fragment_order(seeds, std_sort), split_len=split, split_gap=split)]
                    out.append((alns, anchors))
                except ModelAssertion:
                    out.append(None)
            self._runs[key] = (out, ext)
        return self._runs[key]

    # ---- what the models' results cover
    def trace_letters(self, results):
        """(trace cells, those on ambiguous split nodes, {graph letter outside ACGT: cells on it}) of the whole-read alignments."""
        g, amb = self.graph(), self.ambiguous()
        cells = on_ambiguous = 0
        letters = {}
        for res in results:
            for _, _, _, trace in (res[0] if res else []):
                for node, off, _sp, _sw in trace:
                    split = g.unitig_node(node, off)
                    cells += 1
                    on_ambiguous += amb[split]
                    c = g.sequence[split][off - g.node_offset[split]]
                    if c not in "ACGT":
                        letters[c] = letters.get(c, 0) + 1
        return cells, on_ambiguous, letters

    def anchor_paths(self, results):
        """(anchors, those with an ambiguous split node in their path)."""
        amb = self.ambiguous()
        paths = [path for res in results if res for _, _, _, path in res[1]]
        return len(paths), sum(any(amb[v] for v in path) for path in paths)
