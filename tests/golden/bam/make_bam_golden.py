"""Writes this directory's .bam files and expected.json with tests/bam_model.py's writer: python tests/golden/bam/make_bam_golden.py. The expected (ids, reads, skipped)
are written down here by hand, not read back with the model's reader; tests/test_bam_model.py holds the reader to them. hand.bam's one record is spelled out byte by byte
below, field by field of the record table (SAMv1 section 4.2), without the writer."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bam_model as bm                              # noqa: E402

# One record, flag 0x10: the read "TTGCANC=" is stored reverse-complemented, as "=GNTGCAA".
HAND_RECORD = bytes([
    0x37, 0x00, 0x00, 0x00,    # block_size 55 = 32 fixed + 3 name + 4 cigar + 4 seq + 8 qual + 4 tag
    0xff, 0xff, 0xff, 0xff,    # refID -1
    0xff, 0xff, 0xff, 0xff,    # pos -1
    0x03,                      # l_read_name 3: "r1" and its NUL
    0x00,                      # mapq 0
    0x48, 0x12,                # bin 4680
    0x01, 0x00,                # n_cigar_op 1
    0x14, 0x00,                # flag 0x14: unmapped, reverse strand
    0x08, 0x00, 0x00, 0x00,    # l_seq 8
    0xff, 0xff, 0xff, 0xff,    # next_refID -1
    0xff, 0xff, 0xff, 0xff,    # next_pos -1
    0x00, 0x00, 0x00, 0x00,    # tlen 0
    0x72, 0x31, 0x00,          # read_name "r1\0"
    0x84, 0x00, 0x00, 0x00,    # cigar: 8S = 8 << 4 | 4
    0x04, 0xf8, 0x42, 0x11,    # seq "=GNTGCAA": = 0, G 4 | N 15, T 8 | G 4, C 2 | A 1, A 1
    0x1e, 0x1e, 0x1e, 0x1e, 0x1e, 0x1e, 0x1e, 0x1e,    # qual 30 x 8
    0x4e, 0x4d, 0x43, 0x00,    # tag NM:C:0
])
assert len(HAND_RECORD) - 4 == 32 + 3 + 4 + 4 + 8 + 4 == 55
HAND_HEADER = b"BAM\x01" + bytes([0, 0, 0, 0]) + bytes([0, 0, 0, 0])      # no text, no references

FILES = {
    "hand.bam": {"ids": ["r1"], "reads": ["TTGCANC="], "skipped": 0},
    "plain.bam": {"ids": ["read/1", "read/2 with words", "r3", "r4"], "reads": ["ACGTACGTTGCA", "GATTACA", "", "N"], "skipped": 0},
    "mixed.bam": {"ids": ["fwd", "rev", "codes", "codes/rc", "tagged"],
                  "reads": ["ACGTTGCAAC", "GTTGCAACGT", "=ACMGRSVTWYHKDBN", "NVHDMRWSYKBCGT=", "ACGTACGTACGTACGTACGTACGTACGTACGTA"], "skipped": 2},
}


def build():
    plain = bm.write([(b"read/1", "ACGTACGTTGCA", 4), (b"read/2 with words", "GATTACA", 0), (b"r3", "", 4), (b"r4", "N", 4)])
    mixed = bm.write([
        (b"fwd", "ACGTTGCAAC", 0, (10 << 4,)),
        (b"rev", "ACGTTGCAAC", 0x10, (10 << 4,), b"NMC\x00"),                       # stored as the reverse complement of GTTGCAACGT
        (b"fwd", "ACGT", 0x100, (4 << 4,)),                                         # secondary: left out
        (b"codes", "=ACMGRSVTWYHKDBN", 4),
        (b"codes/rc", "=ACGVMRSWYKHDBN", 0x14),                                     # 15 letters: an odd l_seq on the reverse strand
        (b"fwd", "TTTT", 0x800 | 0x10, (2 << 4 | 5, 4 << 4), b"SAZchr1,5,+,4M,60,0;\x00"),   # supplementary: left out
        (b"tagged", "ACGTACGTACGTACGTACGTACGTACGTACGTA", 4, (), b"RGZgroup\x00mlBC\x02\x00\x00\x00\x07\x09", bytes(range(33))),
    ], block_sizes=(37,), refs=((b"chr1", 1000), (b"chr2", 2000), (b"a", 1)))
    hand = bm.bgzf(HAND_HEADER + HAND_RECORD, (20,))
    return {"hand.bam": hand, "plain.bam": plain, "mixed.bam": mixed}


if __name__ == "__main__":
    for name, data in build().items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    with open(os.path.join(HERE, "expected.json"), "w") as f:
        json.dump(FILES, f, indent=1, sort_keys=True)
        f.write("\n")
