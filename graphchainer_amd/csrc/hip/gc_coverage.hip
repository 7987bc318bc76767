// Coverage of the graph by the final alignments (gc_coverage; --coverage-out / --base-coverage-out). This build's own: the reference stops at one record per alignment,
// and the first thing done with those records is to count how often every segment and every base was aligned to. The counts need only what is already in HBM - the final
// alignments' trace cells - so they are taken there, a fourth reading of the cells the GAF / vg encoder (gc_output.hip) and the corrected reads (gc_corrected.hip) walk.
// Unlike those, the result outlives the batch: bases[segment] (64 bits) and depth[forward base] (32 bits, optional) belong to a gc_coverage handle that every batch of
// every stream set to it adds into, with atomics. The sums are integers: the order of the atomics does not show in them.
//
// k_cov_add: one wave per alignment, 64 cells per step, the cell before the chunk carried in registers. covCovers (gc_coverage_core.hpp) from a lane's own cell and
// its predecessor's; one ballot of the covering lanes, one of the lanes that open a run of the same segment; the opening lane adds the run's length to bases[segment];
// with depth on every covering lane adds 1 to its word (neighbouring lanes, neighbouring words, except across a strand flip where they run the other way).
// A cell outside the graph is not counted and raises *bad (the batch's own cells never are; a caller's traces are checked on the host before they get here).
// k_cov_add<true, ..> (a handle with links; gc_coverage_links_core.hpp): the traversal step. A lane whose node differs from its predecessor's - the lane below, the carry for
// lane 0 - forms the canonical key of the pair, finds it among the graph's sorted link keys by binary search and adds 1 to the link's 64-bit counter. A pair that is no link
// is not counted and raises *bad (4). k_cov_add<false, ..> is the kernel of a handle without links: the step is compiled out, not branched over (DESIGN.md §3.14 has both
// resource lines).
// k_cov_add<.., true> (a handle with the pileup; gc_pileup_core.hpp): the lane also carries its predecessor's seqPos, reads its read letter and - for an aligned pair - the
// graph's letter set, and adds 1 to one channel of the base's 32-byte row: mismatches by read letter, deletions, insertions. Compiled out of the other two instantiations.
// Measured alternative for the depth (difference marks at run ends + a segmented scan in the finish step): see DESIGN.md §10.
//
// The finish step spells both tables on the device, as the GAF encoder spells its text: per segment / per run a line length, a scan, the lines. The runs of the base table
// (maximal stretches of equal non-zero depth inside a segment) are found per tile of 2048 bases: starts and ends counted, scanned over the tiles, then placed.
#include "gc_kernels.hpp"
#include "gc_coverage_core.hpp"
#include "gc_coverage_links_core.hpp"
#include "gc_pileup_core.hpp"
#include "gc_corrected_core.hpp"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace gcdev {

namespace {

constexpr uint32_t COV_TILE_THREADS = 256, COV_TILE_ITEMS = 8, COV_TILE = COV_TILE_THREADS * COV_TILE_ITEMS;

// the set of plain bases of the letter under (bigraph node, offset in the original node), as k_out_encode reads it (gc_output.hip, graphLetterSet): an all-zero column is 'N'
__device__ __forceinline__ uint32_t covLetterSet(const DGraph& dg, int32_t node, uint32_t offset)
{
	const uint32_t split = dg.lookup[dg.lookupOff[node] + (offset >> 6)];
	const uint32_t at = offset & 63u;
	if (split < dg.firstAmbiguous) return 1u << ((dg.nodeSeq[2 * (size_t)split + (at >> 5)] >> ((at & 31u) * 2)) & 3u);
	const uint64_t* p = dg.ambSeq + 4 * (size_t)(split - dg.firstAmbiguous);
	const uint32_t set = (uint32_t)((p[0] >> at) & 1) | (uint32_t)(((p[1] >> at) & 1) << 1) | (uint32_t)(((p[2] >> at) & 1) << 2) | (uint32_t)(((p[3] >> at) & 1) << 3);
	return set ? set : 15u;
}

template <bool LINKS, bool PILEUP>
__global__ void __launch_bounds__(64) k_cov_add(CovGraph g, CovLinks links, const OutJob* __restrict__ jobs, uint32_t nJobs, const uint8_t* __restrict__ keep, const LongCell* __restrict__ cellPool,
	unsigned long long* __restrict__ bases, uint32_t* __restrict__ depth, uint32_t* __restrict__ bad, CovPile pile)
{
	const uint32_t j = blockIdx.x, lane = threadIdx.x;
	if (j >= nJobs || (keep && !keep[j])) return;
	const uint32_t n = jobs[j].cellLen;
	if (n == 0) return;
	const LongCell* cells = cellPool + jobs[j].cellOff;
	int32_t carryNode = 0; uint32_t carryOffset = 0;   // the cell before this chunk's first
	uint32_t carrySeqPos = 0;                          // (PILEUP only)
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t pos = base + lane;
		const bool valid = pos < n;
		const uint32_t nValid = n - base < 64 ? n - base : 64;
		const LongCell c = cells[valid ? pos : n - 1];
		int32_t pNode = __shfl_up(c.node, 1); uint32_t pOffset = __shfl_up(c.offset, 1);
		if (lane == 0) { pNode = carryNode; pOffset = carryOffset; }
		bool covers = valid && covCovers(pos == 0, pNode, pOffset, c.node, c.offset);
		if (PILEUP) {
			// the pileup step (gc_pileup_core.hpp), before the depth: an aligned pair, a deletion or an insertion adds 1 to one channel of the row of the base under the
			// cell. Everything the cell says is checked before it indexes anything: node and offset against the graph, seqPos against the read.
			uint32_t pSeqPos = __shfl_up(c.seqPos, 1);
			if (lane == 0) pSeqPos = carrySeqPos;
			const uint32_t kind = valid ? pileKind(covers, pileMoved(pos == 0, pSeqPos, c.seqPos)) : (uint32_t)PILE_KIND_NOTHING;
			if (kind != PILE_KIND_NOTHING) {
				const uint32_t readLen = jobs[j].readLen;
				if (c.seqPos >= readLen) atomicOr(bad, COV_BAD_SEQPOS);
				else if (c.node >= 0 && (uint32_t)c.node < g.nIds && c.offset < pile.dg.origSize[c.node]) {   // (a cell outside the graph: the step below says so when it covers; an insertion there has no base to count into)
					const uint32_t s = covSegment(c.node);
					const uint64_t s0 = g.segStart[s], len = g.segStart[s + 1] - s0;
					if (c.offset < len) {
						const uint8_t letter = (uint8_t)pile.reads[jobs[j].readOff + c.seqPos];
						const uint32_t graphSet = kind == PILE_KIND_PAIR ? covLetterSet(pile.dg, c.node, c.offset) : 0u;
						const uint32_t channel = pileCellChannel(kind, (c.node & 1) != 0, letter, pile.iupac[letter], graphSet);
						if (channel != PILE_NONE) {
							uint32_t* word = pile.rows + (s0 + covForward(c.node, c.offset, (uint32_t)len)) * PILE_CHANNELS + channel;
							if (atomicAdd(word, 1u) == 0xffffffffu) atomicExch(word, 0xffffffffu);   // (stays full, like the depth word below)
						}
					}
				} else if (!covers) atomicOr(bad, 1u);
			}
			carrySeqPos = __shfl(c.seqPos, (int)nValid - 1);
		}
		uint32_t seg = 0; uint64_t at = 0;
		if (covers) {
			// bounds before anything is indexed with what the cell says
			bool ok = c.node >= 0 && (uint32_t)c.node < g.nIds;
			if (ok) {
				seg = covSegment(c.node);
				const uint64_t s0 = g.segStart[seg], len = g.segStart[seg + 1] - s0;
				ok = c.offset < len;
				if (ok) at = s0 + covForward(c.node, c.offset, (uint32_t)len);
			}
			if (!ok) { covers = false; atomicOr(bad, 1u); }
		}
		const uint64_t coverMask = __ballot(covers);
		const uint32_t prevSeg = __shfl(seg, (int)covPrevCovering(coverMask, lane));
		const bool opens = covOpens(coverMask, lane, seg, prevSeg);
		const uint64_t openMask = __ballot(opens);
		if (opens) atomicAdd(bases + seg, (unsigned long long)covRunLength(coverMask, openMask, lane));
		if (depth && covers && atomicAdd(depth + at, 1u) == 0xffffffffu) atomicExch(depth + at, 0xffffffffu);   // a full word stays full: whoever wraps it puts it back, and the last of any interleaving is such a store
		if (LINKS) {
			// the traversal step: a lane whose node differs from its predecessor's walks a link. Only the sorted keys are indexed, whatever the cell says.
			if (valid && covTraverses(pos == 0, pNode, c.node)) {
				const uint64_t link = covLinkFind(links.keys, links.n, covLinkKey((uint32_t)pNode, (uint32_t)c.node));
				if (link < links.n) atomicAdd(links.counts + link, 1ull); else atomicOr(bad, 4u);
			}
		}
		carryNode = __shfl(c.node, (int)nValid - 1); carryOffset = __shfl(c.offset, (int)nValid - 1);
	}
}

__global__ void __launch_bounds__(256) k_cov_merge(unsigned long long* __restrict__ dstBases, const unsigned long long* __restrict__ srcBases, uint64_t nSegments,
	uint32_t* __restrict__ dstDepth, const uint32_t* __restrict__ srcDepth, uint64_t nDepth, unsigned long long* __restrict__ dstLinks, const unsigned long long* __restrict__ srcLinks, uint64_t nLinks)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (uint64_t i = first; i < nSegments; i += stride) dstBases[i] += srcBases[i];
	for (uint64_t i = first; i < nLinks; i += stride) dstLinks[i] += srcLinks[i];
	for (uint64_t i = first; i < nDepth; i += stride) dstDepth[i] = covSatAdd(dstDepth[i], srcDepth[i]);
}

// ---- the segment table
template <bool WRITE>
__global__ void __launch_bounds__(256) k_cov_segments(CovGraph g, OutNames names, const unsigned long long* __restrict__ bases, uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s > g.nSegments) return;
	if (s == g.nSegments) { if (!WRITE) lens[s] = 0; return; }   // (the scan's last entry is the total)
	const uint32_t id = (uint32_t)(2 * s);
	const uint32_t nameLen = names.nameOff[id + 1] - names.nameOff[id];
	const uint64_t length = g.segStart[s + 1] - g.segStart[s];
	if (!WRITE) lens[s] = covSegmentLineLen(nameLen, s, length, bases[s]);
	else covSegmentLine(text + off[s], names.nameBytes + names.nameOff[id], nameLen, s, length, bases[s]);
}

// ---- the link table and the tagged GFA: rows [first, first + count) of the links / the segments, a thread per row; a row left out (supportedOnly, zero count) has length 0
// KIND 0: the link table's line, 1: the GFA's L line
template <bool WRITE, int KIND>
__global__ void __launch_bounds__(256) k_cov_links(OutNames names, CovLinks links, uint64_t first, uint64_t count, bool supportedOnly, uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > count) return;
	if (r == count) { if (!WRITE) lens[r] = 0; return; }   // (the scan's last entry is the total)
	const uint64_t key = links.keys[first + r], traversals = links.counts[first + r];
	const uint32_t from = covLinkFrom(key), to = covLinkTo(key);
	if (supportedOnly && traversals == 0) { if (!WRITE) lens[r] = 0; return; }
	// (a link's two names are looked up by the segment's forward id, as the segment table does: both strands carry the same name, and an odd id past an odd nIds has none)
	const uint32_t fromId = from & ~1u, toId = to & ~1u;
	const uint32_t fromLen = names.nameOff[fromId + 1] - names.nameOff[fromId], toLen = names.nameOff[toId + 1] - names.nameOff[toId];
	const char* fromName = names.nameBytes + names.nameOff[fromId];
	const char* toName = names.nameBytes + names.nameOff[toId];
	if (!WRITE) lens[r] = KIND == 0 ? covLinkLineLen(fromLen, toLen, from, to, traversals) : covGfaLinkLineLen(fromLen, toLen, from, to, traversals);
	else if (KIND == 0) covLinkLine(text + off[r], fromName, fromLen, toName, toLen, from, to, traversals);
	else covGfaLinkLine(text + off[r], fromName, fromLen, toName, toLen, from, to, traversals);
}

// the S line without its letters (they are k_cov_gfa_letters'): a thread per segment
template <bool WRITE>
__global__ void __launch_bounds__(256) k_cov_gfa_segments(CovGraph g, OutNames names, const unsigned long long* __restrict__ bases, uint64_t first, uint64_t count, bool supportedOnly,
	uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text, uint32_t* __restrict__ bad)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > count) return;
	if (r == count) { if (!WRITE) lens[r] = 0; return; }
	const uint64_t s = first + r;
	if (supportedOnly && bases[s] == 0) { if (!WRITE) lens[r] = 0; return; }
	const uint32_t id = (uint32_t)(2 * s);
	const uint32_t nameLen = names.nameOff[id + 1] - names.nameOff[id];
	const uint64_t length = g.segStart[s + 1] - g.segStart[s];
	if (!WRITE) {
		const uint64_t bytes = covGfaSegmentLineLen(nameLen, s, length, bases[s]);
		if (bytes > 0xffffffffull) atomicOr(bad, 8u);
		lens[r] = (uint32_t)bytes;
	} else covGfaSegmentLine(text + off[r], names.nameBytes + names.nameOff[id], nameLen, s, nullptr, length, bases[s]);
}

// the set of plain bases (A 1, C 2, G 4, T 8) of forward base `pos` of segment s, as gc_corrected.hip reads it; a segment the graph holds only the reverse strand of is read
// there and complemented (the set's four bits reversed)
__device__ __forceinline__ uint32_t covForwardSet(const DGraph& dg, uint32_t nIds, uint64_t s, uint32_t pos, uint32_t length)
{
	uint32_t id = (uint32_t)(2 * s), offset = pos;
	const bool flip = dg.origSize[id] == 0 && id + 1 < nIds;
	if (flip) { id++; offset = length - 1 - pos; }
	const uint32_t split = dg.lookup[dg.lookupOff[id] + (offset >> 6)];
	const uint32_t at = offset & 63u;
	uint32_t set;
	if (split < dg.firstAmbiguous) set = 1u << ((dg.nodeSeq[2 * (size_t)split + (at >> 5)] >> ((at & 31u) * 2)) & 3u);
	else {
		const uint64_t* p = dg.ambSeq + 4 * (size_t)(split - dg.firstAmbiguous);
		set = (uint32_t)((p[0] >> at) & 1) | (uint32_t)(((p[1] >> at) & 1) << 1) | (uint32_t)(((p[2] >> at) & 1) << 2) | (uint32_t)(((p[3] >> at) & 1) << 3);
	}
	return flip ? ((set & 1u) << 3 | (set & 2u) << 1 | (set & 4u) >> 1 | (set & 8u) >> 3) : set;
}

// the letters of the S lines: a thread per forward base of segments [first, first + count), neighbouring threads neighbouring bytes
__global__ void __launch_bounds__(256) k_cov_gfa_letters(CovGraph g, DGraph dg, OutNames names, uint64_t first, uint64_t count, const uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text)
{
	const uint64_t i = g.segStart[first] + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= g.segStart[first + count]) return;
	const uint64_t s = covSegmentOfBase(g.segStart, g.nSegments, i);
	if (s < first || s >= first + count || lens[s - first] == 0) return;   // (a segment left out has no line to write into)
	const uint64_t s0 = g.segStart[s];
	const uint32_t id = (uint32_t)(2 * s);
	const uint32_t nameLen = names.nameOff[id + 1] - names.nameOff[id];
	text[off[s - first] + covGfaSegmentLettersAt(nameLen, s) + (i - s0)] = corrLetter(covForwardSet(dg, g.nIds, s, (uint32_t)(i - s0), (uint32_t)(g.segStart[s + 1] - s0)));
}

// ---- the pileup table: a thread per forward base of [first, first + count); a base that does not pass (pilePasses) has length 0
template <bool WRITE>
__global__ void __launch_bounds__(256) k_cov_pileup(CovGraph g, DGraph dg, OutNames names, const uint32_t* __restrict__ depth, const uint32_t* __restrict__ rows, uint64_t first, uint64_t count, uint64_t minAlt, double minFraction,
	uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > count) return;
	if (r == count) { if (!WRITE) lens[r] = 0; return; }   // (the scan's last entry is the total)
	const uint64_t i = first + r;
	const uint32_t d = depth[i];
	uint32_t row[PILE_CHANNELS];
	const uint4 lo = *(const uint4*)(rows + i * PILE_CHANNELS), hi = *(const uint4*)(rows + i * PILE_CHANNELS + 4);   // (a row is 32 bytes, aligned as such)
	row[0] = lo.x; row[1] = lo.y; row[2] = lo.z; row[3] = lo.w; row[4] = hi.x; row[5] = hi.y; row[6] = hi.z; row[7] = hi.w;
	if (!pilePasses(d, row, minAlt, minFraction)) { if (!WRITE) lens[r] = 0; return; }
	const uint64_t s = covSegmentOfBase(g.segStart, g.nSegments, i);
	const uint64_t s0 = g.segStart[s];
	const uint32_t id = (uint32_t)(2 * s);
	const uint32_t nameLen = names.nameOff[id + 1] - names.nameOff[id];
	if (!WRITE) lens[r] = pileLineLen(nameLen, s, i - s0, d, row);
	else pileLine(text + off[r], names.nameBytes + names.nameOff[id], nameLen, s, i - s0, corrLetter(covForwardSet(dg, g.nIds, s, (uint32_t)(i - s0), (uint32_t)(g.segStart[s + 1] - s0))), d, row);
}

// ---- the base table: runs per tile
// One thread, COV_TILE_ITEMS consecutive bases: visit(i, starts, ends)
template <typename F>
__device__ __forceinline__ void covWalk(const CovGraph& g, const uint32_t* __restrict__ depth, uint64_t first, F&& visit)
{
	if (first >= g.nBases) return;
	uint64_t s = covSegmentOfBase(g.segStart, g.nSegments, first);
	uint64_t segBegin = g.segStart[s], segEnd = g.segStart[s + 1];
	uint32_t left = first > 0 ? depth[first - 1] : 0, here = depth[first];
	for (uint32_t k = 0; k < COV_TILE_ITEMS; k++) {
		const uint64_t i = first + k;
		if (i >= g.nBases) break;
		while (i >= segEnd) { s++; segBegin = segEnd; segEnd = g.segStart[s + 1]; }   // (empty segments are stepped over)
		const uint32_t right = i + 1 < g.nBases ? depth[i + 1] : 0;
		visit(i, covRunStarts(i == segBegin, left, here), covRunEnds(i + 1 == segEnd, here, right));
		left = here; here = right;
	}
}

template <bool PLACE>
__global__ void __launch_bounds__(COV_TILE_THREADS) k_cov_tiles(CovGraph g, const uint32_t* __restrict__ depth, uint64_t nTiles, uint32_t* __restrict__ tileStarts, uint32_t* __restrict__ tileEnds,
	const uint64_t* __restrict__ tileStartOff, const uint64_t* __restrict__ tileEndOff, uint64_t* __restrict__ runStart, uint64_t* __restrict__ runEnd)
{
	using Scan = hipcub::BlockScan<uint32_t, COV_TILE_THREADS>;
	__shared__ typename Scan::TempStorage tmpA, tmpB;
	const uint64_t tile = blockIdx.x;
	const uint64_t first = tile * COV_TILE + (uint64_t)threadIdx.x * COV_TILE_ITEMS;
	uint32_t nStarts = 0, nEnds = 0;
	covWalk(g, depth, first, [&](uint64_t, bool st, bool en) { nStarts += st; nEnds += en; });
	uint32_t startsBefore = 0, endsBefore = 0, startsAll = 0, endsAll = 0;
	Scan(tmpA).ExclusiveSum(nStarts, startsBefore, startsAll);
	Scan(tmpB).ExclusiveSum(nEnds, endsBefore, endsAll);
	if (!PLACE) {
		if (threadIdx.x == 0) { tileStarts[tile] = startsAll; tileEnds[tile] = endsAll; if (tile == 0) { tileStarts[nTiles] = 0; tileEnds[nTiles] = 0; } }
		return;
	}
	uint64_t sAt = tileStartOff[tile] + startsBefore, eAt = tileEndOff[tile] + endsBefore;
	covWalk(g, depth, first, [&](uint64_t i, bool st, bool en) { if (st) runStart[sAt++] = i; if (en) runEnd[eAt++] = i + 1; });
}

template <bool WRITE>
__global__ void __launch_bounds__(256) k_cov_runs(CovGraph g, OutNames names, const uint32_t* __restrict__ depth, const uint64_t* __restrict__ runStart, const uint64_t* __restrict__ runEnd, uint64_t nRuns,
	uint32_t* __restrict__ lens, const uint64_t* __restrict__ off, char* __restrict__ text, uint32_t* __restrict__ bad)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > nRuns) return;
	if (r == nRuns) { if (!WRITE) lens[r] = 0; return; }
	const uint64_t b = runStart[r], e = runEnd[r];
	const uint64_t s = covSegmentOfBase(g.segStart, g.nSegments, b);
	const uint64_t s0 = g.segStart[s];
	const uint32_t id = (uint32_t)(2 * s);
	const uint32_t nameLen = names.nameOff[id + 1] - names.nameOff[id];
	if (!WRITE) {
		if (e <= b || e > g.segStart[s + 1]) atomicOr(bad, 2u);   // the k-th start and the k-th end belong to one run inside one segment
		lens[r] = covRunLineLen(nameLen, s, b - s0, e - s0, depth[b]);
	} else covRunLine(text + off[r], names.nameBytes + names.nameOff[id], nameLen, s, b - s0, e - s0, depth[b]);
}

struct Scratch {   // device memory of one finish call
	void* p = nullptr;
	hipError_t get(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
	~Scratch() { if (p) (void)hipFree(p); }
};
#define COV_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// exclusive sums of n 32-bit counts as 64-bit offsets
hipError_t scanCounts(hipStream_t q, const uint32_t* counts, uint64_t* off, uint64_t n)
{
	using Widen = hipcub::TransformInputIterator<uint64_t, hipcub::CastOp<uint64_t>, const uint32_t*>;
	size_t bytes = 0;
	COV_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, Widen(counts, hipcub::CastOp<uint64_t>()), off, (int)n, q));
	Scratch tmp;
	COV_TRY(tmp.get(bytes));
	COV_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, Widen(counts, hipcub::CastOp<uint64_t>()), off, (int)n, q));
	return hipStreamSynchronize(q);   // (tmp goes when this returns)
}

// the text and the line offsets down: *text malloc'd (head + the device's bytes, NUL-terminated), *lineOff malloc'd [nLines + 1 (+ 1 with a head line)]
hipError_t bringDown(hipStream_t q, const char* head, const char* dText, uint64_t total, const uint64_t* dOff, uint64_t nLines, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLinesOut)
{
	const uint64_t h = head ? strlen(head) : 0, extra = head ? 1 : 0;
	char* t = (char*)malloc(h + total + 1);
	uint64_t* o = (uint64_t*)malloc((nLines + 1 + extra) * sizeof(uint64_t));
	if (!t || !o) { free(t); free(o); return hipErrorOutOfMemory; }
	if (h) memcpy(t, head, h);
	hipError_t e = total ? hipMemcpyAsync(t + h, dText, total, hipMemcpyDeviceToHost, q) : hipSuccess;
	if (e == hipSuccess) e = hipMemcpyAsync(o + extra, dOff, (nLines + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q);
	if (e == hipSuccess) e = hipStreamSynchronize(q);
	if (e != hipSuccess) { free(t); free(o); return e; }
	if (extra) { o[0] = 0; for (uint64_t i = 1; i <= nLines + 1; i++) o[i] += h; }
	t[h + total] = 0;
	*text = t; *len = h + total; *lineOff = o; *nLinesOut = nLines + extra;
	return hipSuccess;
}

} // namespace

void launchCoverageAdd(hipStream_t stream, const CovGraph& g, const CovLinks& links, const OutJob* jobs, uint32_t nJobs, const uint8_t* keep, const LongCell* cellPool, unsigned long long* bases, uint32_t* depth, uint32_t* bad,
	const CovPile& pile)
{
	if (!nJobs) return;
	const bool l = links.counts != nullptr, p = pile.rows != nullptr;
	auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(nJobs), dim3(64), 0, stream, g, links, jobs, nJobs, keep, cellPool, bases, depth, bad, pile); };
	if (l && p) launch(k_cov_add<true, true>);
	else if (p) launch(k_cov_add<false, true>);
	else if (l) launch(k_cov_add<true, false>);
	else launch(k_cov_add<false, false>);
}

void launchCoverageMerge(hipStream_t stream, unsigned long long* dstBases, const unsigned long long* srcBases, uint64_t nSegments, uint32_t* dstDepth, const uint32_t* srcDepth, uint64_t nDepth,
	unsigned long long* dstLinks, const unsigned long long* srcLinks, uint64_t nLinks)
{
	const uint64_t most = std::max(std::max(nSegments, nDepth), nLinks);
	if (!most) return;
	const uint64_t blocks = (most + 255) / 256;
	hipLaunchKernelGGL(k_cov_merge, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, dstBases, srcBases, nSegments, dstDepth, srcDepth, nDepth, dstLinks, srcLinks, nLinks);
}

hipError_t coverageFormatSegments(hipStream_t q, const CovGraph& g, const OutNames& names, const unsigned long long* bases, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	const uint64_t n = g.nSegments;
	if (n + 1 >= 0x7fffffffull) return hipErrorInvalidValue;
	Scratch lens, off, out;
	COV_TRY(lens.get((n + 1) * sizeof(uint32_t)));
	COV_TRY(off.get((n + 1) * sizeof(uint64_t)));
	const dim3 grid((uint32_t)((n + 1 + 255) / 256));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_segments<false>), grid, dim3(256), 0, q, g, names, bases, (uint32_t*)lens.p, (const uint64_t*)nullptr, (char*)nullptr);
	COV_TRY(scanCounts(q, (const uint32_t*)lens.p, (uint64_t*)off.p, n + 1));
	uint64_t total = 0;
	COV_TRY(hipMemcpyAsync(&total, (uint64_t*)off.p + n, sizeof total, hipMemcpyDeviceToHost, q));
	COV_TRY(hipStreamSynchronize(q));
	COV_TRY(out.get(total));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_segments<true>), grid, dim3(256), 0, q, g, names, bases, (uint32_t*)nullptr, (const uint64_t*)off.p, (char*)out.p);
	COV_TRY(hipGetLastError());
	return bringDown(q, "#segment\tlength\tbases\n", (const char*)out.p, total, (const uint64_t*)off.p, n, text, len, lineOff, nLines);
}

hipError_t coverageFormatBases(hipStream_t q, const CovGraph& g, const OutNames& names, const uint32_t* depth, uint32_t* bad, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	const uint64_t nTiles = (g.nBases + COV_TILE - 1) / COV_TILE;
	if (nTiles + 1 >= 0x7fffffffull) return hipErrorInvalidValue;
	Scratch counts, offs, runs, lens, off, out;
	COV_TRY(counts.get(2 * (nTiles + 1) * sizeof(uint32_t)));
	COV_TRY(offs.get(2 * (nTiles + 1) * sizeof(uint64_t)));
	uint32_t* tileStarts = (uint32_t*)counts.p; uint32_t* tileEnds = tileStarts + nTiles + 1;
	uint64_t* tileStartOff = (uint64_t*)offs.p; uint64_t* tileEndOff = tileStartOff + nTiles + 1;
	uint64_t nRuns = 0, nRunEnds = 0;
	if (nTiles) {
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_tiles<false>), dim3((uint32_t)nTiles), dim3(COV_TILE_THREADS), 0, q, g, depth, nTiles, tileStarts, tileEnds, (const uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
		COV_TRY(scanCounts(q, tileStarts, tileStartOff, nTiles + 1));
		COV_TRY(scanCounts(q, tileEnds, tileEndOff, nTiles + 1));
		COV_TRY(hipMemcpyAsync(&nRuns, tileStartOff + nTiles, sizeof nRuns, hipMemcpyDeviceToHost, q));
		COV_TRY(hipMemcpyAsync(&nRunEnds, tileEndOff + nTiles, sizeof nRunEnds, hipMemcpyDeviceToHost, q));
		COV_TRY(hipStreamSynchronize(q));
	}
	if (nRuns != nRunEnds || nRuns + 1 >= 0x7fffffffull) return hipErrorInvalidValue;   // (as many ends as starts; hipCUB counts in int)
	COV_TRY(runs.get(2 * nRuns * sizeof(uint64_t)));
	uint64_t* runStart = (uint64_t*)runs.p; uint64_t* runEnd = runStart + nRuns;
	if (nRuns) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_tiles<true>), dim3((uint32_t)nTiles), dim3(COV_TILE_THREADS), 0, q, g, depth, nTiles, (uint32_t*)nullptr, (uint32_t*)nullptr, (const uint64_t*)tileStartOff, (const uint64_t*)tileEndOff, runStart, runEnd);
	COV_TRY(lens.get((nRuns + 1) * sizeof(uint32_t)));
	COV_TRY(off.get((nRuns + 1) * sizeof(uint64_t)));
	const dim3 grid((uint32_t)((nRuns + 1 + 255) / 256));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_runs<false>), grid, dim3(256), 0, q, g, names, depth, (const uint64_t*)runStart, (const uint64_t*)runEnd, nRuns, (uint32_t*)lens.p, (const uint64_t*)nullptr, (char*)nullptr, bad);
	COV_TRY(scanCounts(q, (const uint32_t*)lens.p, (uint64_t*)off.p, nRuns + 1));
	uint64_t total = 0; uint32_t flags = 0;
	COV_TRY(hipMemcpyAsync(&total, (uint64_t*)off.p + nRuns, sizeof total, hipMemcpyDeviceToHost, q));
	COV_TRY(hipMemcpyAsync(&flags, bad, sizeof flags, hipMemcpyDeviceToHost, q));
	COV_TRY(hipStreamSynchronize(q));
	if (flags & 2u) return hipErrorInvalidValue;   // starts and ends did not pair up: nothing is written from them
	COV_TRY(out.get(total));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_runs<true>), grid, dim3(256), 0, q, g, names, depth, (const uint64_t*)runStart, (const uint64_t*)runEnd, nRuns, (uint32_t*)nullptr, (const uint64_t*)off.p, (char*)out.p, bad);
	COV_TRY(hipGetLastError());
	return bringDown(q, nullptr, (const char*)out.p, total, (const uint64_t*)off.p, nRuns, text, len, lineOff, nLines);
}

namespace {

// rows left out have no line: their (equal) offsets go, *nLines counts what is left
void dropEmptyLines(uint64_t* lineOff, uint64_t* nLines)
{
	*nLines = (uint64_t)(std::unique(lineOff, lineOff + *nLines + 1) - lineOff) - 1;
}

template <int KIND>
hipError_t formatLinkRows(hipStream_t q, const OutNames& names, const CovLinks& links, uint64_t first, uint64_t count, bool supportedOnly, const char* head, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	if (first > links.n || count > links.n - first || count + 1 >= 0x7fffffffull) return hipErrorInvalidValue;
	Scratch lens, off, out;
	COV_TRY(lens.get((count + 1) * sizeof(uint32_t)));
	COV_TRY(off.get((count + 1) * sizeof(uint64_t)));
	const dim3 grid((uint32_t)((count + 1 + 255) / 256));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_links<false, KIND>), grid, dim3(256), 0, q, names, links, first, count, supportedOnly, (uint32_t*)lens.p, (const uint64_t*)nullptr, (char*)nullptr);
	COV_TRY(scanCounts(q, (const uint32_t*)lens.p, (uint64_t*)off.p, count + 1));
	uint64_t total = 0;
	COV_TRY(hipMemcpyAsync(&total, (uint64_t*)off.p + count, sizeof total, hipMemcpyDeviceToHost, q));
	COV_TRY(hipStreamSynchronize(q));
	COV_TRY(out.get(total));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_links<true, KIND>), grid, dim3(256), 0, q, names, links, first, count, supportedOnly, (uint32_t*)nullptr, (const uint64_t*)off.p, (char*)out.p);
	COV_TRY(hipGetLastError());
	COV_TRY(bringDown(q, head, (const char*)out.p, total, (const uint64_t*)off.p, count, text, len, lineOff, nLines));
	if (supportedOnly) dropEmptyLines(*lineOff, nLines);
	return hipSuccess;
}

} // namespace

hipError_t coverageFormatLinks(hipStream_t q, const OutNames& names, const CovLinks& links, uint64_t first, uint64_t count, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	return formatLinkRows<0>(q, names, links, first, count, false, first == 0 ? "#from\tfrom_orient\tto\tto_orient\ttraversals\n" : nullptr, text, len, lineOff, nLines);
}

hipError_t coverageFormatGfaLinks(hipStream_t q, const OutNames& names, const CovLinks& links, uint64_t first, uint64_t count, bool supportedOnly, char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	return formatLinkRows<1>(q, names, links, first, count, supportedOnly, nullptr, text, len, lineOff, nLines);
}

hipError_t coverageFormatGfaSegments(hipStream_t q, const CovGraph& g, const DGraph& dg, const OutNames& names, const unsigned long long* bases, uint32_t* bad, uint64_t first, uint64_t count, bool supportedOnly,
	char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	if (first > g.nSegments || count > g.nSegments - first || count + 1 >= 0x7fffffffull) return hipErrorInvalidValue;
	Scratch lens, off, out;
	COV_TRY(lens.get((count + 1) * sizeof(uint32_t)));
	COV_TRY(off.get((count + 1) * sizeof(uint64_t)));
	const dim3 grid((uint32_t)((count + 1 + 255) / 256));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_gfa_segments<false>), grid, dim3(256), 0, q, g, names, bases, first, count, supportedOnly, (uint32_t*)lens.p, (const uint64_t*)nullptr, (char*)nullptr, bad);
	COV_TRY(scanCounts(q, (const uint32_t*)lens.p, (uint64_t*)off.p, count + 1));
	uint64_t total = 0, range[2] = { 0, 0 }; uint32_t flags = 0;
	COV_TRY(hipMemcpyAsync(&total, (uint64_t*)off.p + count, sizeof total, hipMemcpyDeviceToHost, q));
	COV_TRY(hipMemcpyAsync(&flags, bad, sizeof flags, hipMemcpyDeviceToHost, q));
	COV_TRY(hipMemcpyAsync(&range[0], g.segStart + first, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
	COV_TRY(hipMemcpyAsync(&range[1], g.segStart + first + count, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
	COV_TRY(hipStreamSynchronize(q));
	if (flags & 8u) return hipErrorInvalidValue;   // a line of 2^32 bytes or more: nothing is written from the counts
	COV_TRY(out.get(total));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_gfa_segments<true>), grid, dim3(256), 0, q, g, names, bases, first, count, supportedOnly, (uint32_t*)nullptr, (const uint64_t*)off.p, (char*)out.p, bad);
	const uint64_t nLetters = range[1] - range[0], blocks = (nLetters + 255) / 256;
	if (blocks >= 0x7fffffffull) return hipErrorInvalidValue;
	if (blocks) hipLaunchKernelGGL(k_cov_gfa_letters, dim3((uint32_t)blocks), dim3(256), 0, q, g, dg, names, first, count, (const uint32_t*)lens.p, (const uint64_t*)off.p, (char*)out.p);
	COV_TRY(hipGetLastError());
	COV_TRY(bringDown(q, nullptr, (const char*)out.p, total, (const uint64_t*)off.p, count, text, len, lineOff, nLines));
	if (supportedOnly) dropEmptyLines(*lineOff, nLines);
	return hipSuccess;
}

hipError_t coverageFormatPileup(hipStream_t q, const CovGraph& g, const DGraph& dg, const OutNames& names, const uint32_t* depth, const uint32_t* rows, uint64_t first, uint64_t count, uint64_t minAlt, double minFraction,
	char** text, uint64_t* len, uint64_t** lineOff, uint64_t* nLines)
{
	if (first > g.nBases || count > g.nBases - first || count + 1 >= 0x7fffffffull) return hipErrorInvalidValue;
	Scratch lens, off, out;
	COV_TRY(lens.get((count + 1) * sizeof(uint32_t)));
	COV_TRY(off.get((count + 1) * sizeof(uint64_t)));
	const dim3 grid((uint32_t)((count + 1 + 255) / 256));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_pileup<false>), grid, dim3(256), 0, q, g, dg, names, depth, rows, first, count, minAlt, minFraction, (uint32_t*)lens.p, (const uint64_t*)nullptr, (char*)nullptr);
	COV_TRY(scanCounts(q, (const uint32_t*)lens.p, (uint64_t*)off.p, count + 1));
	uint64_t total = 0;
	COV_TRY(hipMemcpyAsync(&total, (uint64_t*)off.p + count, sizeof total, hipMemcpyDeviceToHost, q));
	COV_TRY(hipStreamSynchronize(q));
	COV_TRY(out.get(total));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_pileup<true>), grid, dim3(256), 0, q, g, dg, names, depth, rows, first, count, minAlt, minFraction, (uint32_t*)nullptr, (const uint64_t*)off.p, (char*)out.p);
	COV_TRY(hipGetLastError());
	COV_TRY(bringDown(q, first == 0 ? "#segment\tpos\tref\tdepth\tmatch\tmmA\tmmC\tmmG\tmmT\tmmN\tdel\tins_before\tins_after\n" : nullptr, (const char*)out.p, total, (const uint64_t*)off.p, count, text, len, lineOff, nLines));
	dropEmptyLines(*lineOff, nLines);
	return hipSuccess;
}

} // namespace gcdev
