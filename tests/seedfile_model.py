"""The reference's seeds-file reader as a model: the loop of stream::for_each (src/stream.hpp:93-116) followed call by call over an inflated stream, every message parsed by
the protobuf Python runtime through vg_descriptor.alignment_class() - Google's own rules for unknown, repeated and merged fields - and turned into a SeedHit as the lambda at
src/Aligner.cpp:1177-1180 does, with the conversions to gc_seed_hit's 32-bit fields that include/graphchainer_amd.h defines. Where the reference is undefined (a stream that
ends inside a count, a size or a message; a message that does not parse; no mapping; no edit) the model raises SeedFileRefused, as the library returns GC_ERR_INVALID.

Also the writer the tests make their files with: it takes raw serialized messages, so hand-built byte strings go in beside real ones."""
import gzip
import zlib

import vg_descriptor


class SeedFileRefused(Exception):
    pass


def varint(value):
    value &= (1 << 64) - 1
    out = bytearray()
    while True:
        if value < 0x80:
            out.append(value)
            return bytes(out)
        out.append((value & 0x7F) | 0x80)
        value >>= 7


def write_stream(groups):
    """[[message bytes, ...] per group] -> the inflated stream; a group given as an int is a bare count (for the damaged shapes)."""
    out = bytearray()
    for group in groups:
        if isinstance(group, int):
            out += varint(group)
            continue
        out += varint(len(group))
        for message in group:
            out += varint(len(message)) + message
    return bytes(out)


def write_file(path, streams, kind="gzip"):
    """Each element of `streams` becomes one compressed member: several gzip members, or one zlib stream."""
    with open(path, "wb") as f:
        for raw in streams:
            f.write(gzip.compress(raw, 6, mtime=0) if kind == "gzip" else zlib.compress(raw, 6))


def seed_message(name, node_id, offset, seq_pos, length, reverse, Alignment=None):
    """One seed as vg writes it."""
    Alignment = Alignment or vg_descriptor.alignment_class()
    msg = Alignment()
    msg.name = name
    msg.query_position = seq_pos
    mapping = msg.path.mapping.add()
    mapping.position.node_id = node_id
    mapping.position.offset = offset
    mapping.position.is_reverse = bool(reverse)
    mapping.edit.add().from_length = length
    return msg.SerializeToString()


def _read_varint(raw, at, what):
    """CodedInputStream::ReadVarint64: at most 10 bytes, bits beyond the 64th dropped. -> (value, next) or None at a clean end of the stream."""
    value = 0
    for i in range(10):
        if at + i >= len(raw):
            if i == 0:
                return None
            raise SeedFileRefused(f"a {what} is cut by the end of the stream")
        b = raw[at + i]
        value |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return value & ((1 << 64) - 1), at + i + 1
    raise SeedFileRefused(f"a {what} of more than 10 bytes")


def _refuse_groups(data, type_name):
    """Protobuf skips a well-formed unknown group; the library refuses the group wire types (vg.proto has none). Runs on a message protobuf has parsed, so everything in
    front of the first group is well formed; sub-messages of the schema are walked, as the parser walks them."""
    fields = {number: (kind, sub) for _, number, kind, _, sub in vg_descriptor.FIELDS[type_name]}
    at = 0
    while at < len(data):
        tag, at = vg_descriptor.read_varint(data, at)
        wire = tag & 7
        if wire in (3, 4):
            raise SeedFileRefused("a group wire type")
        if wire == 0:
            _, at = vg_descriptor.read_varint(data, at)
        elif wire == 1:
            at += 8
        elif wire == 5:
            at += 4
        else:
            size, at = vg_descriptor.read_varint(data, at)
            kind, sub = fields.get(tag >> 3, (None, None))
            if kind == "message":
                _refuse_groups(data[at:at + size], sub)
            at += size


def hit_of(message, Alignment):
    """(name bytes, (node_id, node_offset, seq_pos, match_len, raw_goodness, reverse)) of one serialized vg::Alignment."""
    from google.protobuf.message import DecodeError
    msg = Alignment()
    try:
        msg.ParseFromString(message)
    except DecodeError as e:
        raise SeedFileRefused(f"a message does not parse: {e}")
    _refuse_groups(message, "Alignment")
    if len(msg.path.mapping) == 0:
        raise SeedFileRefused("a message without a mapping")
    mapping = msg.path.mapping[0]
    if len(mapping.edit) == 0:
        raise SeedFileRefused("a mapping without an edit")
    node_id, offset, seq_pos, length = mapping.position.node_id, mapping.position.offset, msg.query_position, mapping.edit[0].from_length
    node32 = ((node_id + (1 << 31)) % (1 << 32)) - (1 << 31)                 # int64 cut to int
    offset32 = offset if 0 <= offset <= 0xFFFFFFFE else 0xFFFFFFFF          # what gc_seed_hit cannot hold: a value no node has
    seq32 = seq_pos if 0 <= seq_pos <= 0xFFFFFFFE else 0xFFFFFFFF
    len32 = length % (1 << 32)                                              # the int32 read as uint32_t
    return msg.name.encode(), (node32, offset32, seq32, len32, len32, int(mapping.position.is_reverse))


def read_stream(raw, Alignment=None):
    """[(name, hit), ...] in file order."""
    Alignment = Alignment or vg_descriptor.alignment_class()
    out = []
    got = _read_varint(raw, 0, "count")
    if got is None:
        return out                                  # an empty stream has no seeds
    count, at = got
    if not count:
        return out                                  # :97
    while True:                                     # do ... while (:98-116)
        for _ in range(count):
            got = _read_varint(raw, at, "size")
            if got is None:
                raise SeedFileRefused("a count runs past the end of the stream")
            size, at = got
            size &= 0xFFFFFFFF                      # ReadVarint32
            if size > 0:                            # :109
                if at + size > len(raw):
                    raise SeedFileRefused("a size runs past the end of the stream")
                out.append(hit_of(raw[at:at + size], Alignment))
                at += size
        got = _read_varint(raw, at, "count")
        if got is None:
            return out
        count, at = got


def seed_map(streams, Alignment=None):
    """The reference's seedHits map over the -s files in command-line order: name -> hits in file order."""
    Alignment = Alignment or vg_descriptor.alignment_class()
    hits = {}
    for raw in streams:
        for name, hit in read_stream(raw, Alignment):
            hits.setdefault(name, []).append(hit)
    return hits


def inflate(data):
    """A file's bytes -> the inflated stream: gzip or zlib by the header, concatenated members read through."""
    out = bytearray()
    while data:
        d = zlib.decompressobj(47)
        try:
            out += d.decompress(data)
        except zlib.error as e:
            raise SeedFileRefused(f"neither gzip nor zlib: {e}")
        if not d.eof:
            raise SeedFileRefused("the file ends inside a member")
        data = d.unused_data
    return bytes(out)
