// Coverage of the graph by the final alignments (--coverage-out / --base-coverage-out; this build's own, the reference has no counterpart), the parts that compile for the
// host as well as for the device (tests/coverage_host):
//   covCovers       the per-cell rule: cell i of a trace covers the graph base under it iff i == 0 or its (node, offset) differs from cell i-1's. An insertion repeats its
//                   predecessor's position and covers nothing; a match, a mismatch and a deletion cover one base each. (nodeSwitch plays no part: a base is a base.)
//   covForward      the strand flip: the base is reported on segment node / 2 at `offset` for an even bigraph id, at length - 1 - offset for an odd one
//   covOpens / covRunLength   one 64-cell step of a wave: the covering lanes fall into runs of the same segment; the lane that opens a run adds the run's length to
//                   bases[segment] (one 64-bit atomic per run instead of one per cell). The kernel makes the masks with two ballots; the host test runs covChunk over
//                   64 emulated lanes.
//   covRunStarts / covRunEnds   the run rule of the base table: a run is a maximal stretch of equal non-zero depth inside one segment
//   covDecimalLen / covDecimal  the integers of both tables
//   covSatAdd       depth words stop at 2^32 - 1 (gc_coverage_merge)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_COV_HD __host__ __device__ __forceinline__
#else
#define GC_COV_HD inline
#endif

namespace gcdev {

GC_COV_HD bool covCovers(bool first, int32_t prevNode, uint32_t prevOffset, int32_t node, uint32_t offset)
{
	return first || node != prevNode || offset != prevOffset;
}

GC_COV_HD uint32_t covSegment(int32_t node) { return (uint32_t)node >> 1; }
GC_COV_HD uint32_t covForward(int32_t node, uint32_t offset, uint32_t length) { return (node & 1) ? length - 1 - offset : offset; }

// lane l opens a run: it covers, and the nearest covering lane below it (in this chunk) is on another segment or there is none
GC_COV_HD bool covOpens(uint64_t coverMask, uint32_t lane, uint32_t segment, uint32_t segmentOfPrevCovering)
{
	if (!((coverMask >> lane) & 1)) return false;
	const uint64_t below = coverMask & ((1ull << lane) - 1);
	return below == 0 || segment != segmentOfPrevCovering;
}
// the nearest covering lane below `lane` (only asked when there is one)
GC_COV_HD uint32_t covPrevCovering(uint64_t coverMask, uint32_t lane)
{
	const uint64_t below = coverMask & ((1ull << lane) - 1);
	return below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
}
// covering lanes from the opening lane up to the next opening lane
GC_COV_HD uint32_t covRunLength(uint64_t coverMask, uint64_t openMask, uint32_t lane)
{
	const uint64_t above = lane == 63 ? 0 : openMask & ~((2ull << lane) - 1);
	const uint64_t upTo = above ? (1ull << (uint32_t)__builtin_ctzll(above)) - 1 : ~0ull;
	return (uint32_t)__builtin_popcountll(coverMask & upTo & ~((1ull << lane) - 1));
}

struct CovLane { int32_t node; uint32_t offset; };
// One chunk of nValid cells whose first cell has index `base`; carry = the cell before the chunk (unused when base == 0). -> coverMask, openMask
GC_COV_HD void covChunk(const CovLane* lanes, uint32_t nValid, uint32_t base, const CovLane& carry, uint64_t& coverMask, uint64_t& openMask)
{
	coverMask = 0; openMask = 0;
	for (uint32_t l = 0; l < nValid; l++) {
		const CovLane& p = l == 0 ? carry : lanes[l - 1];
		if (covCovers(base + l == 0, p.node, p.offset, lanes[l].node, lanes[l].offset)) coverMask |= 1ull << l;
	}
	for (uint32_t l = 0; l < nValid; l++)
		if (covOpens(coverMask, l, covSegment(lanes[l].node), covSegment(lanes[covPrevCovering(coverMask, l)].node))) openMask |= 1ull << l;
}

// base i of a segment (depthLeft: base i-1's depth, unused for the segment's first base; depthRight likewise for its last)
GC_COV_HD bool covRunStarts(bool firstOfSegment, uint32_t depthLeft, uint32_t depth) { return depth != 0 && (firstOfSegment || depthLeft != depth); }
GC_COV_HD bool covRunEnds(bool lastOfSegment, uint32_t depth, uint32_t depthRight) { return depth != 0 && (lastOfSegment || depthRight != depth); }

GC_COV_HD uint32_t covSatAdd(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s < a ? 0xffffffffu : s; }

GC_COV_HD uint32_t covDecimalLen(uint64_t v)
{
	uint32_t n = 1;
	while (v >= 10) { v /= 10; n++; }
	return n;
}
// writes v at out, returns the digits written
GC_COV_HD uint32_t covDecimal(char* out, uint64_t v)
{
	const uint32_t n = covDecimalLen(v);
	for (uint32_t i = n; i-- > 0;) { out[i] = (char)('0' + v % 10); v /= 10; }
	return n;
}

// the lines of the two tables: name "\t" a "\t" b ["\t" c] "\n"; a segment without a name prints its number (as the GAF path does)
GC_COV_HD uint32_t covNameLen(uint32_t nameLen, uint64_t segment) { return nameLen ? nameLen : covDecimalLen(segment); }
GC_COV_HD uint32_t covName(char* out, const char* name, uint32_t nameLen, uint64_t segment)
{
	if (!nameLen) return covDecimal(out, segment);
	for (uint32_t i = 0; i < nameLen; i++) out[i] = name[i];
	return nameLen;
}
GC_COV_HD uint32_t covSegmentLineLen(uint32_t nameLen, uint64_t segment, uint64_t length, uint64_t bases)
{
	return covNameLen(nameLen, segment) + 1 + covDecimalLen(length) + 1 + covDecimalLen(bases) + 1;
}
GC_COV_HD uint32_t covSegmentLine(char* out, const char* name, uint32_t nameLen, uint64_t segment, uint64_t length, uint64_t bases)
{
	uint32_t at = covName(out, name, nameLen, segment);
	out[at++] = '\t'; at += covDecimal(out + at, length);
	out[at++] = '\t'; at += covDecimal(out + at, bases);
	out[at++] = '\n';
	return at;
}
GC_COV_HD uint32_t covRunLineLen(uint32_t nameLen, uint64_t segment, uint64_t start, uint64_t end, uint32_t depth)
{
	return covNameLen(nameLen, segment) + 1 + covDecimalLen(start) + 1 + covDecimalLen(end) + 1 + covDecimalLen(depth) + 1;
}
GC_COV_HD uint32_t covRunLine(char* out, const char* name, uint32_t nameLen, uint64_t segment, uint64_t start, uint64_t end, uint32_t depth)
{
	uint32_t at = covName(out, name, nameLen, segment);
	out[at++] = '\t'; at += covDecimal(out + at, start);
	out[at++] = '\t'; at += covDecimal(out + at, end);
	out[at++] = '\t'; at += covDecimal(out + at, depth);
	out[at++] = '\n';
	return at;
}

// the segment that holds global base index i: segStart[nSegments + 1] ascends, empty segments allowed (the last s with segStart[s] <= i)
GC_COV_HD uint64_t covSegmentOfBase(const uint64_t* segStart, uint64_t nSegments, uint64_t i)
{
	uint64_t lo = 0, hi = nSegments;   // segStart[lo] <= i < segStart[hi]
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (segStart[mid] <= i) lo = mid; else hi = mid;
	}
	return lo;
}

} // namespace gcdev
