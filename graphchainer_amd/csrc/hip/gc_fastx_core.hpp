// The FASTA / FASTQ loader (gc_reads_parse; the reference's FastQ::streamFastqFromFile, src/fastqloader.h), the parts that compile for the host as well as for the device
// (tests/fastx_host). One chunk of file text is turned into tables by passes that have no serial walk in them:
//   fxLine             a line's start, its length with and without the trailing '\r', its first byte, and whether it ended in '\n'
//   fxFastqMap         FASTQ: the line as a map state -> state of the reader's four states (seek header, sequence, plus, quality), four 2-bit entries in a byte;
//   FxCompose          ... the inclusive scan of the maps under composition gives the state after every line, so the role of every line
//   fxFastaHeader      FASTA: the header flag of a line; the inclusive sum of the flags gives the record of every line
//   fxContribution     the bytes a line gives to the compacted reads (its length if it is a sequence line of a record that is kept, else 0); the exclusive sum of these is
//                      where each line's bytes go, and at a header line it is the read's offset
//   fxRecordCount      how many of the headers are records of this chunk (without FX_FINAL the record whose end has not been seen is left out), fxConsumed: where the next chunk begins
//   fxGatherSpan       the bytes [p0, p1) of the compacted reads, found by a binary search over the lines' destinations: a 10 kb line is spread over many callers and a
//                      caller's span may cross many one-letter lines
// The quirks of the reference's reader that these keep are listed in DESIGN.md §9 (tests/fastx_model.py follows its getline / good() calls literally).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_FX_HD __host__ __device__ __forceinline__
#else
#define GC_FX_HD inline
#endif

namespace gcdev {

enum FxFormat : int32_t { FX_FASTA = 1, FX_FASTQ = 2 };   // GC_FASTX_FASTA / GC_FASTX_FASTQ
constexpr uint32_t FX_FINAL = 1;                           // GC_FASTX_FINAL

constexpr uint32_t FX_BLOCK = 256;                                       // threads per block of every pass
constexpr uint32_t FX_COUNT_BYTES = 16;                                  // newline count: bytes per thread and step (one 128-bit load)
constexpr uint32_t FX_COUNT_TILE = FX_BLOCK * FX_COUNT_BYTES * 8;        // ... bytes per block
constexpr uint32_t FX_GATHER_BYTES = 16;                                 // gather: output bytes per thread (one 128-bit store)
constexpr uint32_t FX_GATHER_TILE = FX_BLOCK * FX_GATHER_BYTES;          // ... per block
constexpr uint32_t FX_NAME_LANES = 64;                                   // ids: one wave per record

struct FxView {
	const char* text;          // [len] the chunk
	uint32_t len;
	uint32_t nNewlines;        // '\n' bytes in the text
	uint32_t nLines;           // nNewlines, plus one for a last line without '\n' when the chunk is final
	int32_t format;
	uint32_t final;
	const uint32_t* lineEnd;   // [nNewlines] the position of every '\n', ascending
};

// the '\n' bytes among the four of a word, exactly (no carries between the bytes)
GC_FX_HD uint32_t fxNewlinesInWord(uint32_t w)
{
	const uint32_t y = w ^ 0x0A0A0A0Au;                                         // a zero byte where the text has '\n'
	const uint32_t zero = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);   // 0x80 in every zero byte
#if defined(__HIP_DEVICE_COMPILE__)
	return (uint32_t)__popc(zero);
#else
	return (uint32_t)__builtin_popcount(zero);
#endif
}

// the counts the device hands back in one small copy
enum FxMeta : uint32_t { FX_META_NEWLINES = 0, FX_META_HEADERS, FX_META_RECORDS, FX_META_BASES, FX_META_CONSUMED, FX_META_SELECTED, FX_META_WORDS = 8 };

struct FxLine {
	uint32_t start, rawLen, len;   // len: without one trailing '\r'
	uint8_t first;                 // first byte (0 for an empty line)
	bool complete;                 // ended in '\n'
};

GC_FX_HD FxLine fxLine(const FxView& v, uint32_t i)
{
	FxLine l;
	l.start = i ? v.lineEnd[i - 1] + 1 : 0;
	l.complete = i < v.nNewlines;
	const uint32_t end = l.complete ? v.lineEnd[i] : v.len;
	l.rawLen = end - l.start;
	l.first = l.rawLen ? (uint8_t)v.text[l.start] : (uint8_t)0;
	l.len = l.rawLen && v.text[end - 1] == '\r' ? l.rawLen - 1 : l.rawLen;
	return l;
}

// FASTQ reader states: 0 looks for a header, 1 reads the sequence line, 2 the plus line, 3 the quality line. In state 0 a line is a header if it ended in '\n' (a header
// found after good() turned false is dropped), is not empty and starts with '@'; the three lines after it are taken whatever they hold.
constexpr uint8_t FX_MAP_IDENTITY = 0xE4;   // 3 2 1 0
GC_FX_HD uint8_t fxFastqMap(const FxLine& l)
{
	const uint32_t fromSeek = l.complete && l.rawLen && l.first == '@' ? 1u : 0u;
	return (uint8_t)(fromSeek | (2u << 2) | (3u << 4) | (0u << 6));
}
GC_FX_HD uint32_t fxMapApply(uint8_t map, uint32_t state) { return (map >> (2 * state)) & 3u; }
struct FxCompose {   // first `a`, then `b`: associative, not commutative
	GC_FX_HD uint8_t operator()(uint8_t a, uint8_t b) const
	{
		return (uint8_t)(fxMapApply(b, fxMapApply(a, 0)) | (fxMapApply(b, fxMapApply(a, 1)) << 2) | (fxMapApply(b, fxMapApply(a, 2)) << 4) | (fxMapApply(b, fxMapApply(a, 3)) << 6));
	}
};
// `scanned`: the composition of the maps of lines 0 .. i; the reader starts in state 0. A line is a header iff the reader is in state 1 after it.
GC_FX_HD bool fxFastqIsHeader(uint8_t scanned) { return fxMapApply(scanned, 0) == 1; }
GC_FX_HD bool fxFastqIsSequence(uint8_t scanned) { return fxMapApply(scanned, 0) == 2; }

// FASTA: a header is a line that starts with '>'. The reader tests good() after every getline but the file's first, so a last line without '\n' is lost, header or not,
// unless it is the file's first line (a chunk that is not final holds no such line at all).
GC_FX_HD bool fxFastaHeader(const FxView& v, const FxLine& l, uint32_t i) { return l.rawLen && l.first == '>' && (l.complete || i == 0); }

// headers -> records of this chunk. Final: every header. Otherwise FASTQ keeps a record whose four lines ended in '\n' (at most the last one does not), FASTA a record whose
// next header has been seen. lastHeaderLine: the line of the last header (any value when there is none).
GC_FX_HD uint32_t fxRecordCount(const FxView& v, uint32_t nHeaders, uint32_t lastHeaderLine)
{
	if (v.final || !nHeaders) return nHeaders;
	if (v.format == FX_FASTQ) return (uint64_t)lastHeaderLine + 3 < v.nLines ? nHeaders : nHeaders - 1;
	return nHeaders - 1;
}

// recIdx: headers among lines 0 .. i (inclusive sum); scanned: FASTQ only
GC_FX_HD uint32_t fxContribution(const FxView& v, const FxLine& l, uint32_t i, uint32_t recIdx, uint32_t nHeaders, uint8_t scanned, bool isHeader)
{
	if (v.format == FX_FASTQ) {
		if (!fxFastqIsSequence(scanned)) return 0;
		return v.final || (uint64_t)i + 2 < v.nLines ? l.len : 0;   // (its header is line i - 1)
	}
	if (!recIdx || isHeader || !l.rawLen) return 0;
	if (!l.complete) return 0;                                       // (final: the last sequence line without '\n' is lost)
	return v.final || recIdx < nHeaders ? l.len : 0;
}

// where the caller's next chunk begins. recLine: line of the header of every record [nHeaders]
GC_FX_HD uint32_t fxConsumed(const FxView& v, uint32_t nHeaders, uint32_t nRecords, const uint32_t* recLine)
{
	if (v.final) return v.len;
	if (!nRecords) return 0;
	if (v.format == FX_FASTQ) return v.lineEnd[recLine[nRecords - 1] + 3] + 1;   // behind the quality line
	return fxLine(v, recLine[nRecords]).start;                                     // at the header that ended the last record
}

// Hands bytes [p0, p1) of the compacted reads to sink(p - p0, byte). dest: [nLines + 1] exclusive sum of the contributions (dest[nLines] = all bytes); a line with no
// contribution shares its destination with the next one, so the last line with dest <= p is the one that holds byte p.
template <typename Sink>
GC_FX_HD void fxGatherSpan(const FxView& v, const uint32_t* dest, uint32_t p0, uint32_t p1, Sink&& sink)
{
	if (p0 >= p1) return;
	uint32_t lo = 0, hi = v.nLines;            // largest i in [0, nLines) with dest[i] <= p0 (dest[0] = 0)
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (dest[mid] <= p0) lo = mid; else hi = mid;
	}
	uint32_t line = lo, lineNext = dest[line + 1];
	uint32_t src = fxLine(v, line).start + (p0 - dest[line]);
	for (uint32_t p = p0; p < p1; p++) {
		if (p >= lineNext) {                   // the next line that gives bytes (p < p1 <= dest[nLines]: there is one)
			do lineNext = dest[++line + 1]; while (p >= lineNext);
			src = fxLine(v, line).start;
		}
		sink(p - p0, v.text[src++]);
	}
}

#if defined(__HIPCC__)
// ---- the device passes (gc_fastx.hip), in the order gc_reads_parse runs them; every array is the caller's ----
struct FxTables {
	uint32_t* lineEnd;      // [nNewlines]
	uint8_t* map;           // [nLines] FASTQ: the lines' maps
	uint8_t* scanned;       // [nLines] FASTQ: their inclusive scan
	uint32_t* hdr;          // [nLines] header flags
	uint32_t* recIdx;       // [nLines] their inclusive sum
	uint32_t* contrib;      // [nLines + 1]
	uint32_t* dest;         // [nLines + 1]
	uint32_t* recLine;      // [nLines] line of every header
	uint32_t* meta;         // [FX_META_WORDS]
	void* temp;             // scratch of the scans
	size_t tempBytes;
};
size_t fxScanTempBytes(uint32_t len, uint32_t nLines);
hipError_t fxCountNewlines(hipStream_t q, const char* text, uint32_t len, uint32_t* meta);
hipError_t fxBuildTables(hipStream_t q, const FxView& v, const FxTables& t);
hipError_t fxBuildRecords(hipStream_t q, const FxView& v, const FxTables& t, uint32_t nHeaders, uint32_t nRecords, uint64_t* readOff, uint32_t* nameLen, uint32_t* nameOff);
hipError_t fxGatherBases(hipStream_t q, const FxView& v, const FxTables& t, uint32_t total, char* bases);
hipError_t fxWriteNames(hipStream_t q, const FxView& v, const FxTables& t, uint32_t nRecords, const uint32_t* nameOff, char* names);
#endif

} // namespace gcdev
