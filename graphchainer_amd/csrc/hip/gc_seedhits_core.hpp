// Caller-supplied seed hits (gc_seeds_upload / gc_align_batch_seeded), the parts that compile for the host as well as for the device (tests/seedhits_host):
//   seedHitResolve   one SeedHit (src/GraphAlignerWrapper.h:14) -> the split node that holds it and the offset in it: GetUnitigNode(2 * nodeID + reverse, nodeOffset)
//                    (src/AlignmentGraph.cpp:832-848) and the subtraction of the split node's nodeOffset (src/GraphAligner.h:250-252), bounds checked before any dependent load
//   seedWindow       the seed window of one fragment position (src/Aligner.cpp:672-679) for seeds whose matchLen differs, by two binary searches
// The lookup table is the one the reverse-strand twins already use (DGraph::origSize / lookupOff / lookup): a host with its own seeds adds no table to the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_SEED_HD __host__ __device__ __forceinline__
#else
#define GC_SEED_HD inline
#endif

namespace gcdev {

struct SeedHit {   // gc_seed_hit of the C ABI (24 bytes)
	int32_t nodeId;        // SeedHit::nodeID: bigraph id / 2
	uint32_t nodeOffset;   // offset in the oriented original node (bigraph id 2 * nodeId + reverse)
	uint32_t seqPos, matchLen, rawGoodness, reverse;
};

// the split nodes of every bigraph node id in offset order: those of id are lookup[lookupOff[id] .. lookupOff[id + 1])
struct SeedLookup {
	const uint32_t* origSize;     // [nBigraph] length of the original node (0: no such node)
	const uint32_t* lookupOff;    // [nBigraph + 1]
	const uint32_t* lookup;
	const uint32_t* nodeOffset;   // [split nodes] offset inside the original node
	uint32_t nBigraph;
};

enum SeedHitStatus : uint32_t { SEED_HIT_OK = 0, SEED_HIT_NO_NODE = 1, SEED_HIT_OFFSET = 2, SEED_HIT_SEQPOS = 3 };

// The split node that contains an offset is unique, so the last split node that starts at or before it is what the reference's guess-and-walk ends on.
GC_SEED_HD uint32_t seedHitResolve(const SeedLookup& g, const SeedHit& h, uint32_t readLen, uint32_t& splitNode, uint32_t& offsetInSplit)
{
	if (h.nodeId < 0 || h.reverse > 1 || (uint64_t)h.nodeId * 2 + h.reverse >= g.nBigraph) return SEED_HIT_NO_NODE;
	const uint32_t id = (uint32_t)h.nodeId * 2 + h.reverse;
	const uint32_t first = g.lookupOff[id], end = g.lookupOff[id + 1];
	if (first >= end) return SEED_HIT_NO_NODE;
	if (h.nodeOffset >= g.origSize[id]) return SEED_HIT_OFFSET;
	if (h.seqPos >= readLen) return SEED_HIT_SEQPOS;
	uint32_t lo = first, hi = end;   // first split node that starts beyond the offset
	while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (g.nodeOffset[g.lookup[mid]] <= h.nodeOffset) lo = mid + 1; else hi = mid; }
	splitNode = g.lookup[lo - 1];   // (lo > first: the id's first split node starts at 0)
	offsetInSplit = h.nodeOffset - g.nodeOffset[splitNode];
	return SEED_HIT_OK;
}

// One step of the 64-lane running maximum (Hillis-Steele): `other` is the value of the lane `distance` below.
GC_SEED_HD uint32_t seedMaxScanStep(uint32_t mine, uint32_t other, uint32_t lane, uint32_t distance) { return lane >= distance && other > mine ? other : mine; }

// The window [sl, sr) of the fragment at read position l over the position-sorted seeds. The reference's pointer sr (src/Aligner.cpp:673) stops at the first seed whose
// end seqPos + matchLen lies beyond l + splitLen, and never goes back: it is the first i whose RUNNING MAXIMUM of the ends exceeds l + splitLen, and a running maximum is sorted.
// sl (:675) waits at sr and otherwise is the first seed at or after l. endMax(i) = max over j <= i of seqPos[j] + matchLen[j]; key(i) = seqPos[i].
template <class EndMax, class Key>
GC_SEED_HD void seedWindow(EndMax endMax, Key key, uint32_t nSeeds, uint64_t l, uint32_t splitLen, uint32_t& sl, uint32_t& sr)
{
	uint32_t lo = 0, hi = nSeeds;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)endMax(mid) <= l + splitLen) lo = mid + 1; else hi = mid; }
	sr = lo;
	lo = 0; hi = sr;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)key(mid) < l) lo = mid + 1; else hi = mid; }
	sl = lo;
}

} // namespace gcdev
