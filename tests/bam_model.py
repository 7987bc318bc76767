"""Unaligned BAM for the loader's tests: a writer and a reader, each written from the specification's field tables (SAMv1 section 4.2, as include/graphchainer_amd.h
restates them) and from nothing else - not from each other, and not from csrc/hip/gc_bam_core.hpp.

Neither htslib nor samtools exists where these tests are written or where they run. So the pin is the specification restated twice: the writer packs the fields with
struct in the table's order, the reader slices them by the table's offsets, and tests/golden/bam/make_bam_golden.py spells one record out byte by byte a third time. What
real files add beyond the tables (aux tag encodings, the header text's @-lines, bin and mapq values) is stepped over by the loader by size alone, so it does not bear on it.

File header (only at the start of a file):  "BAM\\1" | l_text u32 | text[l_text] | n_ref u32 | n_ref x (l_name u32 | name[l_name] | l_ref u32)
Record:  block_size u32 (the bytes behind it) | refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 | l_seq u32 | next_refID i32 |
         next_pos i32 | tlen i32 | read_name[l_read_name] (NUL-terminated, the NUL counted) | cigar u32 x n_cigar_op | seq[(l_seq + 1) / 2] | qual[l_seq] | tags
Base i: the high nibble of seq[i / 2] for even i, the low nibble for odd i; nibble values spell "=ACMGRSVTWYHKDBN". All integers little-endian."""
import struct

import bgzf_model

LETTERS = "=ACMGRSVTWYHKDBN"
MAGIC = b"BAM\x01"
REVERSE, SECONDARY, SUPPLEMENTARY = 0x10, 0x100, 0x800
# the complement by the letters' meaning (IUPAC sets of A, C, G, T), not by their codes: the loader does it in nibble space
COMPLEMENT = {"=": "=", "A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "S": "S", "W": "W", "V": "B", "B": "V", "H": "D", "D": "H", "N": "N"}


class BamRefused(ValueError):
    """What the loader answers with GC_ERR_INVALID: .record is the record's index in the stream (None for the header), .offset its byte offset."""

    def __init__(self, record, offset, why):
        super().__init__(f"record {record} at byte {offset}: {why}")
        self.record, self.offset, self.why = record, offset, why


# ---- the writer ----
def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    """refs: (name bytes without NUL, length) - an unaligned file has none, an aligned one that is fed here has some."""
    out = MAGIC + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for name, length in refs:
        out += struct.pack("<I", len(name) + 1) + name + b"\x00" + struct.pack("<I", length)
    return out


def pack_seq(seq):
    codes = [LETTERS.index(c) for c in seq] + [0]
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))


def record(name, seq, flag=4, cigar=(), tags=b"", qual=None):
    """name: bytes without NUL; seq: letters of LETTERS as the file stores them (for flag 0x10 that is the reverse complement of the read); cigar: u32 values."""
    name = name if isinstance(name, bytes) else name.encode()
    qual = bytes([0xff]) * len(seq) if qual is None else qual
    assert len(qual) == len(seq) and len(name) + 1 <= 255 and len(cigar) <= 0xffff
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + b"\x00" + b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + qual + tags
    return struct.pack("<I", len(body)) + body


def stream(records, text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    """The inflated bytes of a file: header and records ((name, seq, flag, cigar, tags, qual) tuples, the tail of a tuple may be left out)."""
    return header(text, refs) + b"".join(record(*r) for r in records)


def write(records, block_sizes=(65280,), text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=(), eof=True):
    """A .bam file: the stream cut into BGZF blocks whose text sizes cycle through block_sizes, and the end-of-file block."""
    return bgzf(stream(records, text, refs), block_sizes, eof)


def bgzf(data, block_sizes=(65280,), eof=True):
    out, at, k = [], 0, 0
    while at < len(data):
        size = block_sizes[k % len(block_sizes)]
        out.append(bgzf_model.write(data[at:at + size], block_size=size, eof=False))
        at, k = at + size, k + 1
    return b"".join(out) + (bgzf_model.EOF if eof else b"")


def random_records(rng, n, max_len=80, letters="ACGT"):
    """n records for the writer: lengths from 0 on, every flag this loader looks at, CIGAR ops and tag bytes of any size."""
    out = []
    for k in range(n):
        length = rng.choice((0, 1, 2, 15, 16, 17, 31, 32, 33, rng.randrange(max_len + 1)))
        name = bytes(rng.randrange(33, 127) for _ in range(rng.choice((1, 2, 7, 30))))
        flag = rng.choice((0, 4, 0x10, 0x14, 0x100, 0x800, 0x110, 0x4 | 0x40, 0x10 | 0x80 | 0x200))
        cigar = tuple(rng.randrange(1 << 32) for _ in range(rng.choice((0, 0, 1, 3))))
        out.append((name, "".join(rng.choice(letters) for _ in range(length)), flag, cigar, rng.randbytes(rng.choice((0, 0, 5, 40))), rng.randbytes(length)))
    return out


def damaged(good_record, what):
    """One record's bytes with one field set so that the loader refuses it for `what` (BamRefused.why)."""
    b = bytearray(good_record)
    block_size, l_read_name = int.from_bytes(b[0:4], "little"), b[12]
    if what == "block_size":
        b[0:4] = struct.pack("<I", 31)
    elif what == "name":                       # the last byte of the name is not NUL
        b[36 + l_read_name - 1] = ord("x")
    elif what == "name0":
        b[12] = 0
    elif what == "l_seq":
        b[20:24] = struct.pack("<I", 1 << 31)
    elif what == "span":                       # one base more than the block holds
        b[20:24] = struct.pack("<I", block_size)
    else:
        raise KeyError(what)
    return bytes(b)


# ---- the reader ----
def revcomp(seq):
    return "".join(COMPLEMENT[c] for c in reversed(seq))


def read_header(data):
    """-> the offset behind the header, or None where the end of data cuts it; BamRefused for a wrong magic."""
    if len(data) < 4:
        return None
    if data[:4] != MAGIC:
        raise BamRefused(None, 0, "magic")
    if len(data) < 8:
        return None
    at = 8 + int.from_bytes(data[4:8], "little")
    if at + 4 > len(data):
        return None
    n_ref = int.from_bytes(data[at:at + 4], "little")
    at += 4
    for _ in range(n_ref):
        if at + 4 > len(data):
            return None
        at += 4 + int.from_bytes(data[at:at + 4], "little") + 4
        if at > len(data):
            return None
    return at


def read_record(data, at, index):
    """The record at data[at:] -> (next offset, (id, read) or None for one that is left out); None where the end of data cuts it."""
    if at + 4 > len(data):
        return None
    block_size = int.from_bytes(data[at:at + 4], "little")
    if block_size < 32:
        raise BamRefused(index, at, "block_size")
    if at + 4 + block_size > len(data):
        return None
    b = data[at + 4:at + 4 + block_size]
    l_read_name, n_cigar_op, flag, l_seq = b[8], int.from_bytes(b[12:14], "little"), int.from_bytes(b[14:16], "little"), int.from_bytes(b[16:20], "little")
    if l_read_name == 0:
        raise BamRefused(index, at, "name")
    if l_seq >= 1 << 31:
        raise BamRefused(index, at, "l_seq")
    if 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) // 2 + l_seq > block_size:
        raise BamRefused(index, at, "span")
    name = b[32:32 + l_read_name]
    if name[-1] != 0:
        raise BamRefused(index, at, "name")
    seq_at = 32 + l_read_name + 4 * n_cigar_op
    packed = b[seq_at:seq_at + (l_seq + 1) // 2]
    seq = "".join(LETTERS[packed[i // 2] >> 4 if i % 2 == 0 else packed[i // 2] & 15] for i in range(l_seq))
    nxt = at + 4 + block_size
    if flag & (SECONDARY | SUPPLEMENTARY):
        return nxt, None
    return nxt, (name[:-1], revcomp(seq) if flag & REVERSE else seq)


def read_stream(data, has_header=True, final=True):
    """The loader's answer for these inflated bytes: (ids, reads, skipped, consumed). BamRefused where it refuses; under final a cut header or record is refused too."""
    at = 0
    if has_header:
        at = read_header(data)
        if at is None:
            if final:
                raise BamRefused(None, 0, "cut")
            return [], [], 0, 0
    ids, reads, skipped, index = [], [], 0, 0
    while at < len(data):
        got = read_record(data, at, index)
        if got is None:
            if final:
                raise BamRefused(index, at, "cut")
            break
        at, read = got
        index += 1
        if read is None:
            skipped += 1
        else:
            ids.append(read[0])
            reads.append(read[1])
    return ids, reads, skipped, at


def inflate(file_bytes):
    """The text of a whole BGZF file, block by block with zlib."""
    import zlib
    out, at = [], 0
    for size in bgzf_model.bgzf_sizes(file_bytes):
        out.append(zlib.decompress(file_bytes[at:at + size], 31))
        at += size
    return b"".join(out)


def read_file(file_bytes):
    return read_stream(inflate(file_bytes))[:3]
