// Corrected reads (GraphAligner's --corrected-out / --corrected-clipped-out), the parts that compile for the host as well as for the device (tests/corrected_host):
//   corrKeeps       AddCorrected's rule (src/GraphAligner.h:220-231): the piece of an alignment starts with the graph letter of its first trace cell (:225); cell i >= 1 adds
//                   its graph letter unless !cell[i-1].nodeSwitch and cell[i] stands on cell[i-1]'s node and offset (:228) - an insertion, which adds nothing. A deletion
//                   advances in the graph and adds its letter; a repeated position behind a nodeSwitch is kept, as the rule is written (only a cycle could reach it).
//   corrLetter      the letter of a set of plain bases (A 1, C 2, G 4, T 8): TraceItem::graphCharacter (src/GraphAlignerCommon.h:148-153) as AlignmentGraph::NodeSequences
//                   spells it (src/AlignmentGraph.cpp:751-796), IUPAC codes and the 'N' of an all-zero column included
//   corrChunk       one 64-cell step of a wave, lane by lane: which lanes keep their cell and where each kept letter goes. The kernel does this with a ballot and a
//                   prefix popcount; the host test runs the same function over 64 emulated lanes.
//   corrBody        getCorrected (src/ReadCorrection.cpp:38-64) over the pieces of one read, and getLongestOverlap (:22-36) with its indexing as written. maxOverlap is
//                   getDBGoverlap(), 0 for the 0M graphs this build loads, so nothing is ever trimmed; the parameter stays so that the rule is the reference's.
//   corrRecord / corrClippedRecord   the two FASTA records (writeCorrectedToQueue / writeCorrectedClippedToQueue, src/Aligner.cpp:313-374)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_CORR_HD __host__ __device__ __forceinline__
#else
#define GC_CORR_HD inline
#endif

namespace gcdev {

GC_CORR_HD bool corrKeeps(bool first, int32_t prevNode, uint32_t prevOffset, uint32_t prevSwitch, int32_t node, uint32_t offset)
{
	if (first) return true;                                                      // src/GraphAligner.h:225
	return !(prevSwitch == 0 && offset == prevOffset && node == prevNode);       // :228
}

// index = A | C << 1 | G << 2 | T << 3
GC_CORR_HD char corrLetter(uint32_t set)
{
	// a 64-bit constant per half instead of a table in memory: sixteen letters, eight to a word
	const uint64_t lo = 0x565352474D43414Eull;   // "NACMGRSV"
	const uint64_t hi = 0x4E42444B48595754ull;   // "TWYHKDBN"
	const uint32_t k = set & 7u;
	return (char)(((set & 8u) ? hi : lo) >> (8 * k));
}

// What one lane of a 64-cell step knows: its cell and the one before it (lane 0's predecessor is the last cell of the previous chunk, or nothing at cell 0)
struct CorrLane { int32_t node; uint32_t offset; uint32_t nodeSwitch; };
// keep mask of a chunk of nValid cells whose first cell has index `base`; carry = the cell before the chunk (unused when base == 0)
GC_CORR_HD uint64_t corrKeepMask(const CorrLane* lanes, uint32_t nValid, uint32_t base, const CorrLane& carry)
{
	uint64_t mask = 0;
	for (uint32_t l = 0; l < nValid; l++) {
		const CorrLane& p = l == 0 ? carry : lanes[l - 1];
		if (corrKeeps(base + l == 0, p.node, p.offset, p.nodeSwitch, lanes[l].node, lanes[l].offset)) mask |= 1ull << l;
	}
	return mask;
}
// place of lane l's letter among the chunk's kept letters
GC_CORR_HD uint32_t corrRank(uint64_t keepMask, uint32_t lane) { return (uint32_t)__builtin_popcountll(keepMask & ((1ull << lane) - 1)); }

} // namespace gcdev

// ---- the record assembly: host functions, whichever compiler reads this
#include <cctype>
#include <string>
#include <vector>

namespace gcdev {

struct CorrPiece { uint64_t start, end; const char* text; uint64_t len; };   // Correction (src/ReadCorrection.h): startIndex, endIndex, corrected

inline size_t corrLongestOverlap(const std::string& left, const char* right, size_t rightLen, size_t maxOverlap)   // src/ReadCorrection.cpp:22-36
{
	if (left.size() < maxOverlap) maxOverlap = left.size();
	if (rightLen < maxOverlap) maxOverlap = rightLen;
	for (size_t i = maxOverlap; i > 0; i--) {
		bool match = true;
		for (size_t a = 0; a < i && match; a++) if (left[left.size() - maxOverlap + a] != right[a]) match = false;   // (sic: the window starts maxOverlap back, not i)
		if (match) return i;
	}
	return 0;
}

inline void corrAppend(std::string& out, const char* p, uint64_t n, bool upper)
{
	const size_t at = out.size();
	out.resize(at + n);
	for (uint64_t i = 0; i < n; i++) out[at + i] = (char)(upper ? toupper((unsigned char)p[i]) : tolower((unsigned char)p[i]));
}

// getCorrected (src/ReadCorrection.cpp:38-64): appended to `out`
inline void corrBody(std::string& out, const char* raw, uint64_t rawLen, const std::vector<CorrPiece>& pieces, size_t maxOverlap)
{
	const size_t bodyBegin = out.size();
	uint64_t currentEnd = 0;
	for (const CorrPiece& c : pieces) {
		if (c.start < currentEnd) {                                                        // :45-49
			const size_t overlap = maxOverlap ? corrLongestOverlap(out.substr(bodyBegin), c.text, c.len, maxOverlap) : 0;
			corrAppend(out, c.text + overlap, c.len - overlap, true);
		} else {
			if (c.start > currentEnd) corrAppend(out, raw + currentEnd, (c.start < rawLen ? c.start : rawLen) - (currentEnd < rawLen ? currentEnd : rawLen), false);   // :50-53 (substr clamps)
			corrAppend(out, c.text, c.len, true);                                          // :53,58
		}
		currentEnd = c.end;                                                                // :60 (even when that moves it backwards)
	}
	if (currentEnd < rawLen) corrAppend(out, raw + currentEnd, rawLen - currentEnd, false);   // :62
}

// ">" id "\n" body "\n" (src/Aligner.cpp:340-341); a read without alignments is its lower-cased self (:984)
inline void corrRecord(std::string& out, const std::string& id, const char* raw, uint64_t rawLen, const std::vector<CorrPiece>& pieces, size_t maxOverlap)
{
	out += '>'; out += id; out += '\n';
	corrBody(out, raw, rawLen, pieces, maxOverlap);
	out += '\n';
}
// ">" id "_" i "_" start "_" end "\n" piece "\n" (src/Aligner.cpp:365-366): the piece as AddCorrected left it, not upper-cased again
inline void corrClippedRecord(std::string& out, const std::string& id, size_t index, const CorrPiece& c)
{
	out += '>'; out += id; out += '_'; out += std::to_string(index); out += '_'; out += std::to_string(c.start); out += '_'; out += std::to_string(c.end); out += '\n';
	out.append(c.text, c.len);
	out += '\n';
}

} // namespace gcdev
