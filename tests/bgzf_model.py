"""BGZF as bgzip and htslib write it, for the inflater's tests: a writer with a block size parameter (blocks of a few hundred bytes), the expected bytes from Python's zlib,
and a bit writer for deflate streams made by hand - the refusals of csrc/hip/gc_inflate_core.hpp, one stream each."""
import random
import struct
import zlib

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the 28-byte empty block that ends a BGZF file


def deflate_raw(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def frame(cdata, crc, isize):
    """One BGZF block around a deflate stream: the 18-byte header with BSIZE, the stream, CRC-32 and ISIZE."""
    size = 18 + len(cdata) + 8
    assert size <= 65536
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + cdata + struct.pack("<II", crc & 0xffffffff, isize)


def block(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    return frame(deflate_raw(data, level, mem, strategy), zlib.crc32(data), len(data))


def write(data, block_size=65280, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """data as a chain of blocks of block_size bytes of text (a piece whose block would pass 64 KiB is halved), and the EOF block."""
    out, todo = [], [data[k:k + block_size] for k in range(0, len(data), block_size)]
    while todo:
        piece = todo.pop(0)
        cdata = deflate_raw(piece, level, mem, strategy)
        if 18 + len(cdata) + 8 > 65536:
            todo[:0] = [piece[:len(piece) // 2], piece[len(piece) // 2:]]
        else:
            out.append(frame(cdata, zlib.crc32(piece), len(piece)))
    return b"".join(out) + (EOF if eof else b"")


def bgzf_sizes(data):
    """The sizes of the blocks of a BGZF file (BSIZE + 1 of every 18-byte header)."""
    sizes, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        sizes.append(struct.unpack_from("<H", data, at + 16)[0] + 1)
        at += sizes[-1]
    assert at == len(data)
    return sizes


def bgzf_count(data):
    return len(bgzf_sizes(data))


def zlib_verdict(member):
    """What zlib makes of one gzip member: its bytes, or None where it refuses it, wants more, or ends before the member's end."""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(member)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


def cdata_of(blk):
    return blk[18:-8]


# ---- deflate streams by hand ----
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        """A field: lowest bit first."""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def code(self, code, n):
        """A Huffman code: highest bit first."""
        for k in range(n - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths {symbol: length}."""
    codes, code = {}, 0
    for n in range(1, 16):
        for s in sorted(s for s, l in lengths.items() if l == n):
            codes[s] = (code, n)
            code += 1
        code <<= 1
    return codes


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic(hlit, hdist, cl_lengths, tokens, final=1):
    """The header of a dynamic block: all 19 code-length lengths, then the tokens (a length 0 .. 15, or (16 | 17 | 18, extra bits' value)) in the code-length code."""
    w = Bits().put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(15, 4)
    for s in CL_ORDER:
        w.put(cl_lengths.get(s, 0), 3)
    codes = canonical(cl_lengths)
    for t in tokens:
        s, extra = t if isinstance(t, tuple) else (t, None)
        w.code(*codes[s])
        if extra is not None:
            w.put(extra, CL_EXTRA[s])
    return w


def zeros(n):
    """Tokens for n zero lengths, n >= 11."""
    out = []
    while n > 138 + 10:
        out.append((18, 127))
        n -= 138
    if n > 138:
        out.append((18, 0))
        n -= 11
    out.append((18, n - 11))
    return out


CL4 = {0: 2, 16: 2, 18: 2}   # ... and one more symbol of length 2: a complete code-length code


def handmade():
    """{name: (block, bytes zlib gives or None)}: the refusals of section 1 of the issue, the one incomplete code that is accepted, and the match at the largest distance."""
    text = b"@r1\nACGTACGTACGTTTGACCA\n+\nIIIIIIIIIIIIIIIIIII\n" * 3
    good = block(text)
    crc, isize = zlib.crc32(text), len(text)
    out = {}

    def flip(blk, byte, bit):
        return blk[:byte] + bytes([blk[byte] ^ (1 << bit)]) + blk[byte + 1:]

    def raw(cdata, data=b""):
        return frame(cdata + b"", zlib.crc32(data), len(data))

    out["crc bit"] = flip(good, len(good) - 8, 3)
    out["isize bit"] = flip(good, len(good) - 4, 0)
    out["stream past the data"] = frame(cdata_of(good)[:-1], crc, isize)
    out["stream ends early"] = frame(cdata_of(good) + b"\x00", crc, isize)
    out["block type 3"] = raw(b"\x07\x00")
    out["stored len nlen"] = raw(b"\x01\x05\x00\xfa\xfe" + b"hello", b"hello")
    out["hlit 287"] = raw(dynamic(287, 1, {**CL4, 8: 2}, []).bytes() + bytes(8))
    out["hdist 31"] = raw(dynamic(257, 31, {**CL4, 8: 2}, []).bytes() + bytes(8))
    out["repeat 16 first"] = raw(dynamic(257, 1, {**CL4, 8: 2}, [(16, 0)]).bytes() + bytes(8))
    out["repeat past the end"] = raw(dynamic(257, 1, {**CL4, 8: 2}, [(18, 127), (18, 127)]).bytes() + bytes(8))
    out["no end code"] = raw(dynamic(257, 1, {**CL4, 8: 2}, [8] + zeros(257)).bytes() + bytes(8))
    out["over-subscribed"] = raw(dynamic(257, 1, {**CL4, 1: 2}, [1, 1, 1] + zeros(253) + [1, 0]).bytes() + bytes(8))
    out["incomplete"] = raw(dynamic(257, 1, {**CL4, 2: 2}, [2] + zeros(255) + [2, 0]).bytes() + bytes(8))
    out["incomplete code-length code"] = raw(dynamic(257, 1, {0: 2, 16: 2, 18: 3}, []).bytes() + bytes(8))
    # literal 'A' and end of block in 2 bits, length 3 in 1 bit; the distance code is one code of length 1: accepted
    lengths = {**CL4, 1: 3, 2: 3}
    tokens = zeros(65) + [2] + zeros(190) + [2, 1, 1]
    lit = canonical({65: 2, 256: 2, 257: 1})
    out["single distance code"] = raw(dynamic(258, 1, lengths, tokens).code(*lit[65]).code(*lit[257]).code(0, 1).code(*lit[256]).bytes(), b"AAAA")
    out["the other bit of a single distance code"] = raw(dynamic(258, 1, lengths, tokens).code(*lit[65]).code(*lit[257]).code(1, 1).code(*lit[256]).bytes(), b"AAAA")
    out["symbol 286"] = raw(Bits().put(1, 1).put(1, 2).code(0xC6, 8).bytes() + bytes(2))
    out["distance symbol 30"] = raw(Bits().put(1, 1).put(1, 2).code(0x30 + 65, 8).code(1, 7).code(30, 5).code(0, 7).bytes(), b"AAAA")
    out["distance before the block"] = raw(Bits().put(1, 1).put(1, 2).code(0x30 + 65, 8).code(1, 7).code(1, 5).code(0, 7).bytes(), b"AAAA")
    out["distance 32768"] = raw(max_distance_stream(), MAX_DISTANCE_HALF * 2)
    return {name: (blk, zlib_verdict(blk)) for name, blk in out.items()}


MAX_DISTANCE_HALF = random.Random(5).randbytes(32768)


def max_distance_stream():
    """32 768 random bytes as a stored block, then the same bytes again as matches at distance 32 768, the largest there is (zlib's own deflate stops 262 short of it): a
    fixed block of 126 matches of length 258, one of 257 and one of 3. One BGZF block of ISIZE 65 536."""
    w = Bits().put(1, 1).put(1, 2)
    for length in [258] * 126 + [257, 3]:
        if length == 258:
            w.code(0xC5, 8)                                # symbol 285
        elif length == 257:
            w.code(0xC4, 8).put(30, 5)                     # symbol 284: 227 + 5 extra bits
        else:
            w.code(1, 7)                                   # symbol 257
        w.code(29, 5).put(8191, 13)                        # distance symbol 29: 24 577 + 13 extra bits
    w.code(0, 7)
    return b"\x00" + struct.pack("<HH", 32768, 32767) + MAX_DISTANCE_HALF + w.bytes()


ACCEPTED_HANDMADE = {"single distance code": b"AAAA", "distance 32768": MAX_DISTANCE_HALF * 2}
GPU_REFUSALS = ("crc bit", "isize bit", "distance before the block", "over-subscribed", "block type 3", "stored len nlen", "stream past the data")
