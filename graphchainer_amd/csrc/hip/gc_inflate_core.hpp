// The BGZF inflater (gc_bgzf_inflate, gc_reads_parse_bgzf), the parts that compile for the host as well as for the device (tests/inflate_host): one RFC 1951 decoder for
// one BGZF block, the framing of a block, and the CRC-32 by slices.
//   infHeader          a BGZF member's header: 1f 8b 08, FLG exactly 4, a BC subfield with SLEN 2, ISIZE at most 64 KiB; where its deflate data lies, its ISIZE and CRC
//   InfBits            the bit reader: every read is bounded by the block's data; past it the reader yields zero bits and sets INF_INPUT_END
//   infBuild           canonical Huffman tables from code lengths: counts per length, the symbols in code order, and a first-level table indexed by the next bits
//   infDecode          one symbol: the first-level table, and for longer codes the canonical walk bit by bit
//   infBlock           the deflate blocks of one BGZF block into a sink (lit / copy / stored), every write bounded by ISIZE
//   infCrcLane         the CRC-32 of the output by slices: lane l of n takes the l-th slice and returns crc(slice) * x^(8 * bytes behind it) mod P; the XOR over the
//                      lanes is the CRC-32 of the whole (crc(A|B) = crc(A) * x^(8 len B) + crc(B))
// The acceptance rules are zlib's (InfStatus lists the refusals; the one incomplete code accepted is a single code of length 1); a bad block ends with a status, never with
// an access out of range. Every value the decode loop works on is the same in all lanes of a wave: the device runs it in all 64 lanes at once and the sink shares out the
// copies (hip/gc_inflate.hip).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_INF_HD __host__ __device__ __forceinline__
#else
#define GC_INF_HD inline
#endif

namespace gcdev {

enum InfStatus : uint32_t {
	INF_OK = 0,
	INF_BLOCK_TYPE,        // block type 3
	INF_STORED_LEN,        // LEN != ~NLEN
	INF_TOO_MANY_CODES,    // HLIT > 286 or HDIST > 30
	INF_REPEAT_FIRST,      // repeat 16 with no previous length
	INF_REPEAT_PAST_END,   // a repeat that runs past HLIT + HDIST
	INF_NO_END_CODE,       // no code for symbol 256
	INF_OVERSUBSCRIBED,
	INF_INCOMPLETE,
	INF_BAD_CODE,          // bits that are no code of an incomplete or empty code
	INF_BAD_SYMBOL,        // literal/length 286, 287 or distance 30, 31
	INF_DISTANCE,          // a distance that reaches before the block's output
	INF_OUTPUT_SIZE,       // output other than exactly ISIZE bytes
	INF_INPUT_END,         // the data ended inside the stream
	INF_STREAM_END,        // the stream ended before the last byte of the data
	INF_CRC,
	INF_STATUS_COUNT
};

GC_INF_HD const char* infStatusName(uint32_t s)
{
	switch (s) {
	case INF_OK: return "ok";
	case INF_BLOCK_TYPE: return "invalid block type";
	case INF_STORED_LEN: return "invalid stored block lengths";
	case INF_TOO_MANY_CODES: return "too many length or distance symbols";
	case INF_REPEAT_FIRST: return "length repeat with no previous length";
	case INF_REPEAT_PAST_END: return "length repeat past the last code";
	case INF_NO_END_CODE: return "no end-of-block code";
	case INF_OVERSUBSCRIBED: return "over-subscribed code";
	case INF_INCOMPLETE: return "incomplete code";
	case INF_BAD_CODE: return "invalid code";
	case INF_BAD_SYMBOL: return "invalid literal/length or distance symbol";
	case INF_DISTANCE: return "distance too far back";
	case INF_OUTPUT_SIZE: return "output differs from ISIZE";
	case INF_INPUT_END: return "deflate stream runs past the block's data";
	case INF_STREAM_END: return "deflate stream ends before the block's data";
	case INF_CRC: return "CRC-32 differs";
	default: return "unknown";
	}
}

constexpr uint32_t INF_MAX_ISIZE = 65536;    // BGZF: at most 64 KiB of text per block
// The decode loop runs in all lanes of ONE wave and nowhere else in its workgroup: the lanes build the tables by writing the same values to the same LDS words, a plain
// read-modify-write on count[] among them, which is sound only because the lanes of a wave execute in lockstep and no second wave shares the tables. INF_LANES is the
// wave's size and the workgroup's (__launch_bounds__(INF_LANES) in hip/gc_inflate.hip); a workgroup of more waves would need tables per wave.
constexpr uint32_t INF_LANES = 64;           // lanes of the wave, and CRC slices

// ---- framing ----
struct InfBlock {          // one row of the table the kernel takes
	uint64_t inOff;        // of the deflate data in the compressed piece
	uint64_t outOff;       // of the block's text in the output
	uint32_t inLen;        // deflate bytes
	uint32_t isize;
	uint32_t crc;
	uint32_t pad;
};

enum InfFrame : int32_t { INF_FRAME_BLOCK = 0, INF_FRAME_PARTIAL, INF_FRAME_OTHER };

// The member at p[0 .. avail): a whole BGZF block (its size in `size`, the row without outOff in `b`, offsets relative to p), a BGZF block cut by the end, or something else.
GC_INF_HD int32_t infHeader(const uint8_t* p, uint64_t avail, InfBlock& b, uint32_t& size)
{
	size = 0;
	const uint8_t magic[4] = { 0x1f, 0x8b, 0x08, 0x04 };
	for (uint32_t k = 0; k < 4 && k < avail; k++) if (p[k] != magic[k]) return INF_FRAME_OTHER;
	if (avail < 12) return INF_FRAME_PARTIAL;
	const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
	if (avail < 12ull + xlen) return INF_FRAME_PARTIAL;
	uint32_t at = 0, bsize = 0;
	bool found = false;
	while (at + 4 <= xlen) {
		const uint8_t* f = p + 12 + at;
		const uint32_t slen = (uint32_t)f[2] | ((uint32_t)f[3] << 8);
		if (at + 4 + slen > xlen) return INF_FRAME_OTHER;
		if (f[0] == 'B' && f[1] == 'C' && slen == 2 && !found) { bsize = (uint32_t)f[4] | ((uint32_t)f[5] << 8); found = true; }
		at += 4 + slen;
	}
	if (!found || at != xlen) return INF_FRAME_OTHER;
	size = bsize + 1;
	if (size < 12 + xlen + 8) { size = 0; return INF_FRAME_OTHER; }
	if (avail < size) return INF_FRAME_PARTIAL;
	b.inOff = 12 + xlen;
	b.inLen = size - (12 + xlen) - 8;
	const uint8_t* t = p + size - 8;
	b.crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
	b.isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
	b.outOff = 0; b.pad = 0;
	if (b.isize > INF_MAX_ISIZE) { size = 0; return INF_FRAME_OTHER; }   // framed like BGZF but more text than a block holds: another gzip member, the host's
	return INF_FRAME_BLOCK;
}

// ---- bits ----
struct InfBits {
	const uint8_t* in;
	uint32_t len, pos;     // pos: bytes taken into buf
	uint64_t buf;          // the next bits, lowest first; above nbits zeros, or bits of the data's next byte (infRefill)
	uint32_t nbits;
	uint32_t err;
};

GC_INF_HD void infBitsInit(InfBits& b, const uint8_t* in, uint32_t len) { b.in = in; b.len = len; b.pos = 0; b.buf = 0; b.nbits = 0; b.err = INF_OK; }

// At least 56 bits in buf unless the data has ended. Where 8 bytes are left they are read at once: the bits of the word that do not fit stay above nbits (they are the
// data's own next bits and the next refill writes the same bits there again); the last bytes of the data go in one by one, with zeros above them.
GC_INF_HD void infRefill(InfBits& b)
{
	if (b.len - b.pos >= 8) {
		uint64_t w;
		__builtin_memcpy(&w, b.in + b.pos, 8);
		b.buf |= w << b.nbits;
		const uint32_t whole = (63 - b.nbits) >> 3;
		b.pos += whole; b.nbits += whole * 8;
		return;
	}
	while (b.nbits <= 56 && b.pos < b.len) { b.buf |= (uint64_t)b.in[b.pos++] << b.nbits; b.nbits += 8; }
}
// the next n bits (n <= 32) without taking them; zero bits behind the data's end
GC_INF_HD uint32_t infPeek(InfBits& b, uint32_t n)
{
	if (b.nbits < n) infRefill(b);
	return (uint32_t)(b.buf & ((1ull << n) - 1));
}
GC_INF_HD void infDrop(InfBits& b, uint32_t n)
{
	if (b.nbits < n) { b.err = INF_INPUT_END; b.buf = 0; b.nbits = 0; return; }
	b.buf >>= n; b.nbits -= n;
}
GC_INF_HD uint32_t infTake(InfBits& b, uint32_t n) { const uint32_t v = infPeek(b, n); infDrop(b, n); return v; }
GC_INF_HD uint64_t infBitsUsed(const InfBits& b) { return (uint64_t)b.pos * 8 - b.nbits; }

// ---- Huffman tables ----
constexpr uint32_t INF_LEN_BITS = 10, INF_DIST_BITS = 8, INF_CL_BITS = 7;   // first-level tables: literal/length, distance, code lengths (all of its codes)
constexpr uint32_t INF_MAX_LEN_SYMS = 288, INF_MAX_DIST_SYMS = 32;

struct InfCode {
	uint16_t* lut;         // [1 << lutBits] (symbol << 4) | length for a code of at most lutBits bits at every index that starts with it, else 0
	uint16_t* sym;         // the symbols with a code, by length and then by symbol
	uint16_t* count;       // [16] codes of each length
	uint32_t lutBits;
};

struct InfTables {         // one wave's (LDS on the device)
	uint16_t lenLut[1u << INF_LEN_BITS];
	uint16_t distLut[1u << INF_DIST_BITS];      // (the code-length code's table lies here while the lengths are read)
	uint16_t lenSym[INF_MAX_LEN_SYMS];
	uint16_t distSym[INF_MAX_DIST_SYMS];
	uint16_t lenCount[16], distCount[16];
	uint8_t lengths[INF_MAX_LEN_SYMS + INF_MAX_DIST_SYMS];
};

GC_INF_HD InfCode infLenCode(InfTables& t) { return InfCode { t.lenLut, t.lenSym, t.lenCount, INF_LEN_BITS }; }
GC_INF_HD InfCode infDistCode(InfTables& t) { return InfCode { t.distLut, t.distSym, t.distCount, INF_DIST_BITS }; }
GC_INF_HD InfCode infClCode(InfTables& t) { return InfCode { t.distLut, t.distSym, t.distCount, INF_CL_BITS }; }

GC_INF_HD uint32_t infReverse(uint32_t code, uint32_t bits)
{
	uint32_t r = 0;
	for (uint32_t k = 0; k < bits; k++) { r = (r << 1) | (code & 1); code >>= 1; }
	return r;
}

// lengths[n] (each 0 .. 15, n <= 288) -> the code. allowSingle: an incomplete code is accepted if it is one code of length 1 (zlib: literal/length and distance codes, not
// the code-length code); a code with no symbols at all is accepted in the same places and decodes nothing.
GC_INF_HD uint32_t infBuild(const InfCode& c, const uint8_t* lengths, uint32_t n, bool allowSingle)
{
	uint16_t offs[16];
	for (uint32_t l = 0; l < 16; l++) c.count[l] = 0;
	for (uint32_t s = 0; s < n; s++) c.count[lengths[s] & 15]++;
	c.count[0] = 0;
	int32_t left = 1;
	uint32_t maxLen = 0;
	for (uint32_t l = 1; l < 16; l++) {
		left = (left << 1) - (int32_t)c.count[l];
		if (left < 0) return INF_OVERSUBSCRIBED;
		if (c.count[l]) maxLen = l;
	}
	if (left > 0 && !(allowSingle && maxLen <= 1)) return INF_INCOMPLETE;
	offs[1] = 0;
	for (uint32_t l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
	for (uint32_t s = 0; s < n; s++) { const uint32_t l = lengths[s] & 15; if (l) c.sym[offs[l]++] = (uint16_t)s; }   // (at most n entries)
	const uint32_t lutSize = 1u << c.lutBits;
	for (uint32_t i = 0; i < lutSize; i++) c.lut[i] = 0;
	uint32_t code = 0, index = 0;
	for (uint32_t l = 1; l <= c.lutBits; l++) {
		for (uint32_t k = 0; k < c.count[l]; k++, code++, index++) {
			const uint16_t entry = (uint16_t)((c.sym[index] << 4) | l);
			for (uint32_t i = infReverse(code, l); i < lutSize; i += 1u << l) c.lut[i] = entry;   // (code < 2^l: not over-subscribed)
		}
		code <<= 1;
	}
	return INF_OK;
}

// one symbol, or -1 where the bits are no code (and at the data's end)
GC_INF_HD int32_t infDecode(InfBits& b, const InfCode& c)
{
	const uint32_t bits = infPeek(b, 15);
	const uint32_t e = c.lut[bits & ((1u << c.lutBits) - 1)];
	if (e) { infDrop(b, e & 15); return (int32_t)(e >> 4); }
	uint32_t code = 0, first = 0, index = 0;
	for (uint32_t l = 1; l < 16; l++) {
		code |= (bits >> (l - 1)) & 1;
		const uint32_t cnt = c.count[l];
		if (code < first + cnt) {           // (code >= first: the shorter codes were not it)
			infDrop(b, l);
			return (int32_t)c.sym[index + (code - first)];   // (index + cnt <= symbols with a code)
		}
		index += cnt; first = (first + cnt) << 1; code <<= 1;
	}
	return -1;
}

// The sink of infBlock takes the output. pos is the byte's place in the block's text; every call lies inside [0, isize).
//   lit(pos, byte)   copy(pos, len, dist): len bytes from pos - dist, which may overlap   stored(pos, src, n): n bytes of the compressed data
struct InfHostSink {
	uint8_t* out;
	GC_INF_HD void lit(uint32_t pos, uint8_t v) { out[pos] = v; }
	GC_INF_HD void copy(uint32_t pos, uint32_t len, uint32_t dist) { for (uint32_t k = 0; k < len; k++) out[pos + k] = out[pos + k - dist]; }
	GC_INF_HD void stored(uint32_t pos, const uint8_t* src, uint32_t n) { for (uint32_t k = 0; k < n; k++) out[pos + k] = src[k]; }
};

// reads the code lengths of a dynamic block into t.lengths and builds both codes
GC_INF_HD uint32_t infDynamicHeader(InfBits& b, InfTables& t)
{
	const uint32_t hlit = infTake(b, 5) + 257, hdist = infTake(b, 5) + 1, hclen = infTake(b, 4) + 4;
	if (b.err) return b.err;
	if (hlit > 286 || hdist > 30) return INF_TOO_MANY_CODES;
	const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
	for (uint32_t k = 0; k < 19; k++) t.lengths[k] = 0;
	for (uint32_t k = 0; k < hclen; k++) t.lengths[order[k]] = (uint8_t)infTake(b, 3);
	if (b.err) return b.err;
	const InfCode cl = infClCode(t);
	uint32_t st = infBuild(cl, t.lengths, 19, false);
	if (st) return st;
	const uint32_t total = hlit + hdist;
	uint32_t have = 0;
	while (have < total) {
		const int32_t s = infDecode(b, cl);
		if (b.err) return b.err;
		if (s < 0) return INF_BAD_CODE;
		if (s < 16) { t.lengths[have++] = (uint8_t)s; continue; }
		uint32_t value = 0, repeat;
		if (s == 16) {
			if (!have) return INF_REPEAT_FIRST;
			value = t.lengths[have - 1];
			repeat = 3 + infTake(b, 2);
		} else if (s == 17) repeat = 3 + infTake(b, 3);
		else repeat = 11 + infTake(b, 7);
		if (b.err) return b.err;
		if (have + repeat > total) return INF_REPEAT_PAST_END;
		for (uint32_t k = 0; k < repeat; k++) t.lengths[have++] = (uint8_t)value;
	}
	if (!t.lengths[256]) return INF_NO_END_CODE;
	// the distance lengths move behind the 288 places of the literal/length lengths before the code-length code's tables (the distance code's) are overwritten
	for (uint32_t k = 0; k < hdist; k++) t.lengths[INF_MAX_LEN_SYMS + (hdist - 1 - k)] = t.lengths[hlit + (hdist - 1 - k)];
	st = infBuild(infLenCode(t), t.lengths, hlit, true);
	if (st) return st;
	return infBuild(infDistCode(t), t.lengths + INF_MAX_LEN_SYMS, hdist, true);
}

GC_INF_HD void infFixedTables(InfTables& t)
{
	for (uint32_t s = 0; s < 288; s++) t.lengths[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
	for (uint32_t s = 0; s < 32; s++) t.lengths[INF_MAX_LEN_SYMS + s] = 5;
	(void)infBuild(infLenCode(t), t.lengths, 288, true);
	(void)infBuild(infDistCode(t), t.lengths + INF_MAX_LEN_SYMS, 32, true);
}

// The deflate stream in[0 .. inLen) of one BGZF block into the sink; exactly isize bytes, and the stream ends inside the data's last byte. The CRC is the caller's.
template <typename Sink>
GC_INF_HD uint32_t infBlock(const uint8_t* in, uint32_t inLen, uint32_t isize, InfTables& t, Sink& sink)
{
	InfBits b;
	infBitsInit(b, in, inLen);
	uint32_t pos = 0;
	for (;;) {
		const uint32_t last = infTake(b, 1), type = infTake(b, 2);
		if (b.err) return b.err;
		if (type == 3) return INF_BLOCK_TYPE;
		if (type == 0) {
			infDrop(b, b.nbits & 7);
			const uint32_t lens = infTake(b, 32);
			if (b.err) return b.err;
			const uint32_t n = lens & 0xffff;
			if (n != ((~lens >> 16) & 0xffff)) return INF_STORED_LEN;
			b.pos -= b.nbits >> 3; b.nbits = 0; b.buf = 0;            // whole bytes only are left in buf: hand them back
			if (n > b.len - b.pos) return INF_INPUT_END;
			if (n > isize - pos) return INF_OUTPUT_SIZE;
			sink.stored(pos, in + b.pos, n);
			pos += n; b.pos += n;
		} else {
			if (type == 1) infFixedTables(t);
			else { const uint32_t st = infDynamicHeader(b, t); if (st) return st; }
			const InfCode lc = infLenCode(t), dc = infDistCode(t);
			for (;;) {
				const int32_t s = infDecode(b, lc);
				if (b.err) return b.err;
				if (s < 0) return INF_BAD_CODE;
				if (s < 256) {
					if (pos >= isize) return INF_OUTPUT_SIZE;
					sink.lit(pos++, (uint8_t)s);
					continue;
				}
				if (s == 256) break;
				if (s >= 286) return INF_BAD_SYMBOL;
				uint32_t len;
				if (s < 265) len = (uint32_t)s - 254;
				else if (s == 285) len = 258;
				else { const uint32_t e = ((uint32_t)s - 261) >> 2; len = 3 + ((4 + (((uint32_t)s - 261) & 3)) << e) + infTake(b, e); }
				const int32_t d = infDecode(b, dc);
				if (b.err) return b.err;
				if (d < 0) return INF_BAD_CODE;
				if (d >= 30) return INF_BAD_SYMBOL;
				uint32_t dist;
				if (d < 4) dist = (uint32_t)d + 1;
				else { const uint32_t e = ((uint32_t)d >> 1) - 1; dist = 1 + ((2 + ((uint32_t)d & 1)) << e) + infTake(b, e); }
				if (b.err) return b.err;
				if (dist > pos) return INF_DISTANCE;
				if (len > isize - pos) return INF_OUTPUT_SIZE;
				sink.copy(pos, len, dist);
				pos += len;
			}
		}
		if (last) break;
	}
	if (pos != isize) return INF_OUTPUT_SIZE;
	if ((infBitsUsed(b) + 7) / 8 != inLen) return INF_STREAM_END;
	return INF_OK;
}

// ---- CRC-32 (reflected 0xEDB88320) ----
constexpr uint32_t INF_CRC_POLY = 0xEDB88320u;
GC_INF_HD uint32_t infCrcTableEntry(uint32_t i)
{
	uint32_t c = i;
	for (uint32_t k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ INF_CRC_POLY : c >> 1;
	return c;
}
// a * b mod P, both reflected (bit 31 is x^0)
GC_INF_HD uint32_t infMulModP(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {
		if (a & m) p ^= b;
		b = b & 1 ? (b >> 1) ^ INF_CRC_POLY : b >> 1;
	}
	return p;
}
// x^(8 n) mod P
GC_INF_HD uint32_t infXPow8(uint32_t n)
{
	uint32_t r = 1u << 31, sq = 0x00800000u;   // x^0, x^8
	for (; n; n >>= 1) { if (n & 1) r = infMulModP(r, sq); sq = infMulModP(sq, sq); }
	return r;
}
// table: the 256 entries of infCrcTableEntry. Lane `lane` of `lanes`: the CRC-32 of its slice of out[0 .. n), times x^(8 * bytes behind the slice).
GC_INF_HD uint32_t infCrcLane(const uint32_t* table, const uint8_t* out, uint32_t n, uint32_t lane, uint32_t lanes)
{
	const uint32_t slice = (n + lanes - 1) / lanes;
	const uint64_t lo64 = (uint64_t)lane * slice;
	if (lo64 >= n) return 0;
	const uint32_t lo = (uint32_t)lo64, hi = lo + slice < n ? lo + slice : n;
	uint32_t c = 0xffffffffu;
	for (uint32_t p = lo; p < hi; p++) c = table[(c ^ out[p]) & 0xff] ^ (c >> 8);
	c ^= 0xffffffffu;
	return hi < n ? infMulModP(infXPow8(n - hi), c) : c;
}

#if defined(__HIPCC__)
// ---- the device pass (gc_inflate.hip): block i of the table from data + inOff into out + outOff, status[i] an InfStatus ----
hipError_t infLaunch(hipStream_t q, const uint8_t* data, const InfBlock* blocks, uint32_t nBlocks, uint8_t* out, uint32_t* status);
#endif

} // namespace gcdev
