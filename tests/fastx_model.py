"""Model of the reference's read loader (src/fastqloader.h, includeQuality == false), written to follow std::getline and
std::istream::good() step by step, so that every quirk of the original falls out of the same control flow:

  parse(text, fmt, final=True) -> (ids, sequences, consumed)

fmt is "fasta" or "fastq" (what the file name selects, see file_format). With final the text is a whole file (or its last
part) and consumed == len(text). Without it the text is a chunk from the middle of a file (gc_reads_parse without
GC_FASTX_FINAL): only lines that end in a newline count, a record whose end is not yet known is left out, and consumed is the
byte where the next chunk must begin (0 when no record is complete).

One place is defined where the reference is not: its FASTQ branch calls line.back() on an empty sequence or quality line.
Here such a line is simply empty.
"""


class _Stream:
    """The parts of std::istream that std::getline and good() use."""

    def __init__(self, data):
        self.data, self.pos, self.eof, self.fail = data, 0, False, False
        self.terminated = False   # the last getline ended at a newline
        self.line_start = 0       # where the last getline began

    def good(self):
        return not (self.eof or self.fail)

    def getline(self, line):
        """std::getline(stream, line): returns the new value of `line`."""
        self.terminated = False
        self.line_start = self.pos
        if not self.good():       # the sentry fails: failbit, and the string is left as it was
            self.fail = True
            return line
        end = self.data.find(b"\n", self.pos)
        if end < 0:
            line = self.data[self.pos:]
            self.pos = len(self.data)
            self.eof = True
            if not line:
                self.fail = True  # nothing extracted
            return line
        line = self.data[self.pos:end]
        self.pos = end + 1
        self.terminated = True
        return line


def _strip_cr(line):
    return line[:-1] if line and line[-1:] == b"\r" else line   # (line.back() of an empty line: defined as "nothing to strip")


def _fastq(s, out):
    while True:                                   # do {
        line = s.getline(b"")
        if not s.good():
            break
        if len(line) == 0 or line[:1] != b"@":
            if s.good():
                continue
            break
        name = _strip_cr(line)[1:]
        line = s.getline(line)
        complete = s.terminated
        seq = _strip_cr(line)
        line = s.getline(line)
        complete = complete and s.terminated
        line = s.getline(line)
        complete = complete and s.terminated
        out.append((name, seq, complete, s.pos))
        if not s.good():                          # } while (file.good());
            break


def _fasta(s, out):
    line = s.getline(b"")
    while True:                                   # do {
        if len(line) == 0 or line[:1] != b">":
            line = s.getline(line)
            if s.good():
                continue
            break
        name = _strip_cr(line)[1:]
        seq = b""
        complete, resume = False, s.pos
        while True:                               #   do {
            line = s.getline(line)
            if not s.good():
                break
            if len(line) == 0:
                if s.good():
                    continue
                break
            if line[:1] == b">":
                complete, resume = True, s.line_start
                break
            seq += _strip_cr(line)
            if not s.good():                      #   } while (file.good());
                break
        out.append((name, seq, complete, resume))
        if not s.good():                          # } while (file.good());
            break


def parse(text, fmt, final=True):
    text = bytes(text)
    if fmt not in ("fasta", "fastq"):
        raise ValueError("fmt is 'fasta' or 'fastq'")
    whole = len(text)
    if not final:
        text = text[:text.rfind(b"\n") + 1]       # only lines that end in a newline count
    records = []
    (_fastq if fmt == "fastq" else _fasta)(_Stream(text), records)
    if final:
        return [r[0] for r in records], [r[1] for r in records], whole
    done = [r for r in records if r[2]]
    return [r[0] for r in done], [r[1] for r in done], (done[-1][3] if done else 0)


def file_format(path):
    """FastQ::streamFastqFromFile's choice by file name (src/fastqloader.h:98-139): ("fasta" | "fastq" | None, gzipped)."""
    name = str(path)
    gz = len(name) > 3 and name.endswith(".gz")
    if gz:
        name = name[:-3]
    fastq = (len(name) > 6 and name.endswith(".fastq")) or (len(name) > 3 and name.endswith(".fq"))
    fasta = (len(name) > 6 and name.endswith(".fasta")) or (len(name) > 3 and name.endswith(".fa"))
    return ("fasta" if fasta else "fastq" if fastq else None), gz


ALPHABET = b"\n\r@>+ACGTN "
TILE_SIZES = (16, 64, 256, 4096, 32768)   # every tile of hip/gc_fastx.hip: bytes per thread, lanes per id, threads per block, bytes per block of the gather / a count step, of the count


def random_texts(seed=20261, small=560):
    """Seeded texts over ALPHABET for the host program and the device: `small` of 0-200 bytes, and one of every length t - 1, t, t + 1 around 1x, 2x, 3x every tile
    size. Some are plain noise with few or many newlines, some are records of either format with a few bytes damaged, so that every state of both readers is reached
    deep inside a text as well as at its ends."""
    import random
    rng = random.Random(seed)
    bases = b"ACGTN"

    def noise(n):
        p = rng.choice((0.5, 0.2, 0.06, 0.01))
        return bytes(10 if rng.random() < p else ALPHABET[rng.randrange(1, len(ALPHABET))] for _ in range(n))

    def records(n):
        out, eol = bytearray(), rng.choice((b"\n", b"\n", b"\r\n"))
        fastq, width = rng.random() < 0.5, rng.choice((1, 2, 7, 60, 1000))
        while len(out) < n:
            seq = bytes(rng.choice(bases) for _ in range(rng.choice((0, 1, 3, 17, 64, 150, 700))))
            name = bytes(rng.choice(b"ab \t1") for _ in range(rng.randrange(0, 6)))
            if fastq:
                out += b"@" + name + eol + seq + eol + b"+" + eol + bytes(rng.choice(b"@>I+") for _ in seq) + eol
            else:
                out += b">" + name + eol + b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))
            if rng.random() < 0.2:
                out += rng.choice((b"\n", b"junk\n", b"\r\n", b"@\n", b">\n"))
        out = out[:n]
        for _ in range(rng.choice((0, 0, 1, 3))):
            if out:
                out[rng.randrange(len(out))] = rng.choice(ALPHABET)
        return bytes(out)

    lengths = [rng.randrange(0, 201) for _ in range(small)] + [k * t + d for t in TILE_SIZES for k in (1, 2, 3) for d in (-1, 0, 1)]
    return [(noise if rng.random() < 0.4 else records)(n) for n in lengths]


def parse_chunks(text, fmt, cuts):
    """The chunk protocol: the text arrives in pieces that end at `cuts` (ascending byte positions); every piece but the last
    is parsed without final, what it did not consume is carried over to the next."""
    text = bytes(text)
    ids, seqs, begin = [], [], 0
    for cut in cuts:
        i, s, used = parse(text[begin:cut], fmt, final=False)
        ids += i
        seqs += s
        begin += used
    i, s, _ = parse(text[begin:], fmt, final=True)
    return ids + i, seqs + s
