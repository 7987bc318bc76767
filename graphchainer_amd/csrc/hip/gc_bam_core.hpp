// Unaligned BAM to a read batch (gc_reads_parse_bam), the parts that compile for the host as well as for the device (tests/bam_host). The format is SAMv1 §4.2 as
// include/graphchainer_amd.h restates it, little-endian throughout; positions are 32-bit (the callers keep the bytes below 2^32 - 16), sums of them 64-bit.
//   bamWalk        the file header (with BAM_HEADER) and the chain of block_size words: the start of every whole record, the byte behind the last one, and the one thing
//                  that stops the chain - a wrong magic, a block_size below 32, or under BAM_FINAL a header or record that the end of the bytes cuts. It reads through a
//                  Reader (u32 at a byte position), which on the device is a window in LDS that the whole wave refills
//   bamFields      one record's fixed fields -> its status, whether it is kept (flag 0x100 and 0x800 are left out), l_seq, the strand, and where its name and its
//                  packed bases lie
//   bamUnpackSpan  letters [p0, p1) of the compacted reads (at most 16) from the kept records' spans: a binary search for the read, then 16 letters from 8 bytes at once
//                  where they lie in one read at an even base, else letter by letter; a reverse-strand record is written from its far end, complemented in nibble
//                  space (the 4-bit reversal: A=1 <-> T=8, C=2 <-> G=4, M=3 <-> K=12, ...; '=' and N stay)
// Qualities, CIGAR and tags are stepped over by the sizes alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_BAM_HD __host__ __device__ __forceinline__
#else
#define GC_BAM_HD inline
#endif

namespace gcdev {

constexpr uint32_t BAM_FINAL = 1, BAM_HEADER = 2;          // GC_FASTX_FINAL / GC_BAM_HEADER
constexpr uint32_t BAM_MAGIC_WORD = 0x014D4142u;           // "BAM\1"
constexpr uint32_t BAM_FIXED = 32;                         // the bytes of a record between block_size and read_name
constexpr uint32_t BAM_FLAG_REVERSE = 0x10, BAM_FLAG_LEFT_OUT = 0x100 | 0x800;   // secondary and supplementary records: `samtools fastq` leaves them out by default

constexpr uint32_t BAM_BLOCK = 256;                        // threads per block of the per-record and per-letter passes
constexpr uint32_t BAM_WINDOW = 16384;                     // walk: bytes of LDS the wave reads the chain through
constexpr uint32_t BAM_UNPACK_LETTERS = 16;                // unpack: letters per thread (one 128-bit store)
constexpr uint32_t BAM_NAME_LANES = 8;                     // ids: lanes per record

enum BamStatus : uint32_t { BAM_OK = 0, BAM_BAD_MAGIC, BAM_BAD_BLOCK_SIZE, BAM_BAD_NAME, BAM_BAD_LSEQ, BAM_BAD_SPAN, BAM_CUT, BAM_STATUS_COUNT };
constexpr uint32_t BAM_STATUS_BITS = 3;
inline const char* bamStatusName(uint32_t s)
{
	static const char* const names[BAM_STATUS_COUNT] = { "ok", "the magic is not BAM\\1", "block_size is below 32", "l_read_name is 0 or the name does not end in NUL",
		"l_seq is 2^31 or more", "name, CIGAR, bases and qualities do not fit block_size", "the bytes end inside it" };
	return s < BAM_STATUS_COUNT ? names[s] : "?";
}
// the first refused record of a call, kept by an atomic minimum: (record << BAM_STATUS_BITS) | status; BAM_NONE_REFUSED when there is none
constexpr unsigned long long BAM_NONE_REFUSED = ~0ull;

GC_BAM_HD uint32_t bamU16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
GC_BAM_HD uint32_t bamU32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct BamBytes {   // the host's Reader, and the device's where the bytes are read once
	const uint8_t* p;
	GC_BAM_HD uint32_t u32(uint32_t at) const { return bamU32(p + at); }
};

// n whole records, consumed: the byte behind the last of them (behind the header where there is none; 0 when not even the header is whole). status != BAM_OK: record n
// (the header when inHeader) at byte badAt stops the chain.
struct BamWalk { uint32_t n, consumed, status, badAt, inHeader; };

// the end of the bytes cuts what begins at `at`: refused under BAM_FINAL, left for the next chunk otherwise
GC_BAM_HD void bamCut(BamWalk& w, uint32_t flags, uint64_t at) { if (flags & BAM_FINAL) { w.status = BAM_CUT; w.badAt = (uint32_t)at; } }

// emit(k, start): record k begins at byte `start` (its block_size word)
template <typename Reader, typename Emit>
GC_BAM_HD BamWalk bamWalk(Reader& rd, uint32_t len, uint32_t flags, Emit&& emit)
{
	BamWalk w { 0, 0, BAM_OK, 0, 0 };
	uint64_t pos = 0;
	if (flags & BAM_HEADER) {                               // magic, l_text, text, n_ref, n_ref x (l_name, name, l_ref): stepped over whole
		w.inHeader = 1;
		if (len < 4) { bamCut(w, flags, 0); return w; }
		if (rd.u32(0) != BAM_MAGIC_WORD) { w.status = BAM_BAD_MAGIC; return w; }
		if (len < 8) { bamCut(w, flags, 0); return w; }
		pos = 8 + (uint64_t)rd.u32(4);
		if (pos + 4 > len) { bamCut(w, flags, 0); return w; }
		const uint32_t nRef = rd.u32((uint32_t)pos);
		pos += 4;
		for (uint32_t r = 0; r < nRef; r++) {
			if (pos + 4 > len) { bamCut(w, flags, 0); return w; }
			pos += 4 + (uint64_t)rd.u32((uint32_t)pos) + 4;    // l_name, name, l_ref
			if (pos > len) { bamCut(w, flags, 0); return w; }
		}
		w.inHeader = 0;
		w.consumed = (uint32_t)pos;
	}
	while (pos < len) {
		if (pos + 4 > len) { bamCut(w, flags, pos); return w; }
		const uint32_t blockSize = rd.u32((uint32_t)pos);
		if (blockSize < BAM_FIXED) { w.status = BAM_BAD_BLOCK_SIZE; w.badAt = (uint32_t)pos; return w; }
		if (pos + 4 + blockSize > len) { bamCut(w, flags, pos); return w; }
		emit(w.n, (uint32_t)pos);
		w.n++;
		pos += 4 + (uint64_t)blockSize;
		w.consumed = (uint32_t)pos;
	}
	return w;
}

// a kept record's spans: lSeqRev = l_seq | reverse << 31 (l_seq is below 2^31)
struct BamSpan { uint32_t seqAt, lSeqRev, nameAt, nameLen; };
struct BamRecord { uint32_t status, keep; BamSpan span; };

// the record whose block_size word lies at text[start]; the walk has seen that block_size >= 32 and that the whole block lies inside the bytes
GC_BAM_HD BamRecord bamFields(const uint8_t* text, uint32_t start)
{
	const uint8_t* p = text + start;
	const uint32_t blockSize = bamU32(p), lName = p[12], nCigar = bamU16(p + 16), flag = bamU16(p + 18), lSeq = bamU32(p + 20);
	BamRecord r { BAM_OK, 0, { 0, 0, 0, 0 } };
	if (!lName) { r.status = BAM_BAD_NAME; return r; }
	if (lSeq >= 0x80000000u) { r.status = BAM_BAD_LSEQ; return r; }
	if ((uint64_t)BAM_FIXED + lName + 4ull * nCigar + (lSeq + 1) / 2 + lSeq > blockSize) { r.status = BAM_BAD_SPAN; return r; }
	if (p[4 + BAM_FIXED + lName - 1] != 0) { r.status = BAM_BAD_NAME; return r; }
	r.keep = flag & BAM_FLAG_LEFT_OUT ? 0u : 1u;
	r.span.nameAt = start + 4 + BAM_FIXED;
	r.span.nameLen = lName;                                // with its NUL
	r.span.seqAt = r.span.nameAt + lName + 4 * nCigar;
	r.span.lSeqRev = lSeq | (flag & BAM_FLAG_REVERSE ? 0x80000000u : 0u);
	return r;
}

GC_BAM_HD uint8_t bamLetter(uint32_t nibble)   // "=ACMGRSVTWYHKDBN"
{
	const uint64_t half = nibble & 8 ? 0x4E42444B48595754ull : 0x565352474D43413Dull;
	return (uint8_t)(half >> (8 * (nibble & 7)));
}
GC_BAM_HD uint32_t bamComplement(uint32_t nibble) { return (nibble & 1) << 3 | (nibble & 2) << 1 | (nibble & 4) >> 1 | (nibble & 8) >> 3; }

// letter j of a read as it is written: base j of the record, or for a reverse-strand record the complement of base l_seq - 1 - j
GC_BAM_HD uint8_t bamReadLetter(const uint8_t* text, const BamSpan& s, uint32_t j)
{
	const uint32_t lSeq = s.lSeqRev & 0x7fffffffu, rev = s.lSeqRev >> 31, b = rev ? lSeq - 1 - j : j;
	const uint32_t byte = text[s.seqAt + (b >> 1)], nibble = b & 1 ? byte & 15 : byte >> 4;
	return bamLetter(rev ? bamComplement(nibble) : nibble);
}

// Hands letters [p0, p1) of the compacted reads to sink(p - p0, letter); p1 - p0 <= 16 and p1 <= readOff[nKept]. readOff: [nKept + 1] the kept reads' offsets; a read of
// length 0 shares its offset with the next one, so the last read with readOff <= p is the one that holds letter p.
template <typename Sink>
GC_BAM_HD void bamUnpackSpan(const uint8_t* text, const BamSpan* spans, const uint64_t* readOff, uint32_t nKept, uint64_t p0, uint64_t p1, Sink&& sink)
{
	if (p0 >= p1) return;
	uint32_t lo = 0, hi = nKept;               // largest k in [0, nKept) with readOff[k] <= p0 (readOff[0] = 0)
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (readOff[mid] <= p0) lo = mid; else hi = mid;
	}
	uint32_t k = lo;
	uint64_t next = readOff[k + 1];
	BamSpan s = spans[k];
	uint32_t j = (uint32_t)(p0 - readOff[k]);
	if (p1 - p0 == BAM_UNPACK_LETTERS && p1 <= next) {
		const uint32_t lSeq = s.lSeqRev & 0x7fffffffu, rev = s.lSeqRev >> 31, b0 = rev ? lSeq - BAM_UNPACK_LETTERS - j : j;   // the lowest of the 16 bases
		if (!(b0 & 1)) {                       // they are 8 whole bytes
			uint64_t w = 0;
			for (uint32_t i = 0; i < 8; i++) w |= (uint64_t)text[s.seqAt + (b0 >> 1) + i] << (8 * i);
			for (uint32_t t = 0; t < BAM_UNPACK_LETTERS; t++) {
				const uint32_t b = rev ? BAM_UNPACK_LETTERS - 1 - t : t, byte = (uint32_t)(w >> (8 * (b >> 1))) & 0xffu, nibble = b & 1 ? byte & 15 : byte >> 4;
				sink(t, bamLetter(rev ? bamComplement(nibble) : nibble));
			}
			return;
		}
	}
	for (uint64_t p = p0; p < p1; p++) {
		if (p >= next) {                       // the next read that has letters (p < p1 <= readOff[nKept]: there is one)
			do next = readOff[++k + 1]; while (p >= next);
			s = spans[k];
			j = 0;
		}
		sink((uint32_t)(p - p0), bamReadLetter(text, s, j++));
	}
}

#if defined(__HIPCC__)
// ---- the device passes (gc_bam.hip), in the order gc_reads_parse_bam runs them; every array is the caller's ----
enum BamMeta : uint32_t { BAM_META_RECORDS = 0, BAM_META_CONSUMED, BAM_META_WALK_STATUS, BAM_META_WALK_BAD_AT, BAM_META_IN_HEADER, BAM_META_KEPT, BAM_META_BASES, BAM_META_NAME_BYTES,
	BAM_META_REFUSED_LO, BAM_META_REFUSED_HI, BAM_META_WORDS = 16 };   // REFUSED: one 64-bit word, 8-byte aligned
struct BamTables {
	const uint32_t* recStart;   // [nRecords] from the walk
	uint32_t* keep;             // [nRecords + 1] 1 for a record that becomes a read (the last entry 0), ...
	uint32_t* seqLen;           // [nRecords + 1] ... its l_seq, ...
	uint32_t* nameLen;          // [nRecords + 1] ... its l_read_name; 0 for the others
	uint32_t* kept;             // [nRecords + 1] exclusive sums of the three
	uint32_t* seqOff;
	uint32_t* nameOffAll;
	BamSpan* spansAll;          // [nRecords]
	BamSpan* spans;             // [kept] the kept records', compacted
	uint64_t* readOff;          // [kept + 1] (64-bit, what the packing kernels take)
	uint32_t* nameOff;          // [kept + 1]
	uint32_t* meta;             // [BAM_META_WORDS]
	void* temp;                 // scratch of the scans
	size_t tempBytes;
};
size_t bamScanTempBytes(uint32_t nRecords);
hipError_t bamWalkRecords(hipStream_t q, const uint8_t* text, uint32_t len, uint32_t flags, uint32_t* recStart, uint32_t* meta);
hipError_t bamBuildRecords(hipStream_t q, const uint8_t* text, uint32_t nRecords, const BamTables& t);
hipError_t bamWriteNames(hipStream_t q, const uint8_t* text, uint32_t nRecords, const BamTables& t, char* names);
hipError_t bamUnpackBases(hipStream_t q, const uint8_t* text, const BamTables& t, uint32_t nKept, uint32_t total, char* bases);
#endif

} // namespace gcdev
