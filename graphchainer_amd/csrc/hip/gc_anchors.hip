// The fragment pass around its extensions: the work items built on the device (k_build_fragment_work) and the anchor post-pass (K3b).
#include "gc_kernels.hpp"

namespace gcdev {

// =====================================================================================================
// K3b - fragment post-pass: merges the two one-way traces of every seed, replays the reference's serial
// "seed already lies on an earlier alignment" filter inside each fragment, and emits anchors.
// reference: AlignOneWay src/GraphAligner.h:114-203 (non-sloppy), exactAlignmentPart :407-461,
// getAlignmentFromSeed :567-626, anchor construction src/Aligner.cpp:706-729. One lane per fragment.
// =====================================================================================================

struct MergedView {   // virtual view of a seed's merged trace (backward cells, then forward cells) in forward-strand split coords
	const PoolCell* bw; uint32_t nBw;   // backward device trace without its final row -1 cell (nBw cells used)
	const PoolCell* fw; uint32_t nFw;   // forward device trace (used in reverse order)
	int32_t p;                            // seed position inside the fragment
	__device__ uint32_t size() const { return nBw + nFw; }
};

// cell i of the merged trace: (split node, offset in split node, seqPos in fragment)
__device__ inline void mergedCell(const DGraph& g, const MergedView& v, uint32_t i, uint32_t& node, uint32_t& offset, int32_t& seqPos)
{
	if (i < v.nBw) {
		const PoolCell& c = v.bw[i];
		// backward rows count away from the seed: row b -> fragment position p-1-b (fixReverseTraceSeqPosAndOrder, :543-565)
		seqPos = v.p - 1 - c.seqPos;
		// reverse-strand twin of the cell (GetReversePosition + GetUnitigNode)
		uint32_t off = c.offsetAndSwitch & 255u;
		int32_t id = g.nodeIDs[c.node];
		uint32_t orig = g.nodeOffset[c.node] + off;
		uint32_t rev = g.origSize[id] - 1 - orig;
		uint32_t twin = g.lookup[g.lookupOff[id ^ 1] + rev / 64];
		node = twin;
		offset = rev - g.nodeOffset[twin];
	} else {
		const PoolCell& c = v.fw[v.nFw - 1 - (i - v.nBw)];
		seqPos = v.p + 1 + c.seqPos;   // row -1 -> p
		node = c.node;
		offset = c.offsetAndSwitch & 255u;
	}
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) k_build_anchors(DGraph g, const Fragment* __restrict__ frags, uint32_t nFrags, const FragSeed* __restrict__ seeds,
	const ExtResult* __restrict__ ext, const PoolCell* __restrict__ tracePool, int32_t splitLen,
	AnchorRec* __restrict__ anchors, uint32_t* __restrict__ fragStatus, uint32_t* __restrict__ fragExtended,
	uint32_t* __restrict__ pathPool, unsigned long long* __restrict__ pathCursor, uint64_t pathCapacity, AnchorRounds rounds, uint32_t* __restrict__ readTies)
{
	GC_RAISE_PRIO();
	// Lazy extension (rounds.lazy): a seed's two extensions run only when the reference would run them, i.e. when the seed does not lie on an
	// earlier alignment of its fragment (on cfg2 more than half of the seeds do). Round 0 has the first seed of every fragment extended and
	// walks all fragments; a fragment that reaches a seed it must extend and whose extensions have not run yet parks itself - the seed's
	// two work items go to the next round's list, the fragment to the next round's pending list - and resumes there in the next round.
	uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (rounds.lazy && rounds.round > 0) {
		if (f >= (uint32_t)*rounds.pendingCount) return;
		f = rounds.pending[f];
	} else if (f >= nFrags) return;
	Fragment fr = frags[f];
	uint32_t status = 0;       // 0 ok, 1 the reference would throw in this fragment, 2 capacity overflow
	uint32_t extended = 0;
	// (extensions consumed in this launch whose flattenLastSliceEnd minimum was tied between nodes - ExtResult::pad, one in thirty - are added to the read's count where they are met:
	// a counter kept across the seed loop cost six registers and a wave per SIMD)
	uint32_t nSeeds = fr.seedEnd - fr.seedBegin;
	uint32_t firstSeed = 0;
	if (rounds.lazy && rounds.round > 0) { firstSeed = rounds.fragNext[f]; extended = fragExtended[f]; }
	else for (uint32_t k = 0; k < nSeeds; k++) anchors[fr.seedBegin + k].valid = 0;
	for (uint32_t k = firstSeed; k < nSeeds && status == 0; k++) {
		uint32_t sIdx = fr.seedBegin + k;
		FragSeed sd = seeds[sIdx];
		int32_t p = (int32_t)sd.seqPos - (int32_t)fr.l;
		// --- filter: does the seed cell lie on an earlier accepted alignment of this fragment? (:163-173)
		bool skip = false, haveTwin = false;
		uint32_t twinNode = 0, twinOffset = 0;
		for (uint32_t a = 0; a < k && !skip && status == 0; a++) {
			const AnchorRec& prev = anchors[fr.seedBegin + a];
			if (!prev.valid) continue;
			if (!(prev.lastSeqPos > prev.firstSeqPos)) { status = 1; break; }   // assert at :412
			if ((int32_t)prev.lastSeqPos < p || (int32_t)prev.firstSeqPos > p) continue;
			FragSeed ps = seeds[fr.seedBegin + a];
			const ExtResult& pb = ext[2 * (size_t)(fr.seedBegin + a)];
			const ExtResult& pf = ext[2 * (size_t)(fr.seedBegin + a) + 1];
			MergedView v;
			v.p = (int32_t)ps.seqPos - (int32_t)fr.l;
			bool hasB = pb.status == EXT_OK && v.p > 0, hasF = pf.status == EXT_OK && v.p < splitLen - 1;
			v.bw = tracePool + pb.traceOff; v.nBw = hasB ? (hasF ? pb.traceLen - 1 : pb.traceLen) : 0;
			v.fw = tracePool + pf.traceOff; v.nFw = hasF ? pf.traceLen : 0;
			// Is (seed node, seed offset, p) a cell of this alignment? Only the cells of read position p can be, and a one-way trace's rows never
			// increase along it: a binary search finds them (the reference searches by seqPos too, :415-437; r2 walked every cell of every earlier
			// alignment - 23 GB fetched per 10 k reads, each backward cell through the five gathers of the strand flip). Backward cells are
			// compared on their own strand, against the seed's reverse-strand twin (the flip is a bijection), computed once per seed.
			if (v.nBw > 0) {
				const int32_t row = v.p - 1 - p;   // backward row of read position p
				if (!haveTwin) { twinOf(g, sd.node, sd.offset, twinNode, twinOffset); haveTwin = true; }
				uint32_t lo = 0, hi = v.nBw;      // first cell with seqPos <= row
				while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (v.bw[mid].seqPos > row) lo = mid + 1; else hi = mid; }
				for (uint32_t i = lo; i < v.nBw && !skip; i++) {
					const PoolCell c = v.bw[i];
					if (c.seqPos != row) break;
					if (c.node == twinNode && (c.offsetAndSwitch & 255u) == twinOffset) skip = true;
				}
			}
			if (v.nFw > 0 && !skip) {
				const int32_t row = p - v.p - 1;   // forward row of read position p (row -1 is the seed's own position)
				uint32_t lo = 0, hi = v.nFw;
				while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (v.fw[mid].seqPos > row) lo = mid + 1; else hi = mid; }
				for (uint32_t i = lo; i < v.nFw && !skip; i++) {
					const PoolCell c = v.fw[i];
					if (c.seqPos != row) break;
					if (c.node == sd.node && (c.offsetAndSwitch & 255u) == sd.offset) skip = true;
				}
			}
		}
		if (skip || status != 0) continue;
		// --- this seed is extended: getAlignmentFromSeed (:567-626)
		const ExtResult& eb = ext[2 * (size_t)sIdx];
		const ExtResult& ef = ext[2 * (size_t)sIdx + 1];
		if (rounds.lazy && eb.status == EXT_NOT_RUN) {   // (both directions are queued together, so one test covers both)
			// (the last parking round queues all the seeds the fragment has left: the few fragments that get this far then finish in one more
			// round, at the price of some extensions the reference would not have run)
			const uint32_t nQueued = rounds.parkAll ? nSeeds - k : 1u;
			const unsigned long long at = atomicAdd(rounds.nextListCount, 2ull * nQueued);
			for (uint32_t q = 0; q < nQueued; q++) {
				rounds.nextList[at + 2 * q] = 2 * (sIdx + q);
				rounds.nextList[at + 2 * q + 1] = 2 * (sIdx + q) + 1;
			}
			rounds.nextPending[atomicAdd(rounds.nextPendingCount, 1ull)] = f;
			rounds.fragNext[f] = k;
			fragExtended[f] = extended;
			return;
		}
		extended++;
		bool runB = p > 0, runF = p < splitLen - 1;
		// (the reference runs the backward extension first and the forward one only if that did not throw, src/GraphAligner.h:499-511)
		if (readTies && runB && (eb.pad & 1u)) atomicAdd(&readTies[fr.read], 1u);
		if (readTies && runF && !(runB && eb.status == EXT_ASSERT) && (ef.pad & 1u)) atomicAdd(&readTies[fr.read], 1u);
		if ((runB && eb.status == EXT_ASSERT) || (runF && ef.status == EXT_ASSERT)) { status = 1; break; }
		if ((runB && eb.status == EXT_OVERFLOW) || (runF && ef.status == EXT_OVERFLOW)) { status = 2; break; }
		bool hasB = runB && eb.status == EXT_OK, hasF = runF && ef.status == EXT_OK;
		if (!hasB && !hasF) continue;   // emptyAlignment: alignmentFailed()
		MergedView v;
		v.p = p;
		v.bw = tracePool + eb.traceOff; v.nBw = hasB ? (hasF ? eb.traceLen - 1 : eb.traceLen) : 0;
		v.fw = tracePool + ef.traceOff; v.nFw = hasF ? ef.traceLen : 0;
		uint32_t n = v.size();
		// anchor path = distinct consecutive split nodes along the trace (src/Aligner.cpp:714-720). ONE pass over the two traces (r3): a 35-row fragment crosses one to three
		// split nodes, so the path collects in six registers and only a longer one walks the traces a second time; the cells are fetched eight at a time (twelve-byte cells at a
		// per-lane stride: the eight loads of a group go out together and use a cache line while it is there - issued one per iteration, every load found its line evicted by the
		// other waves' lines and the kernel fetched 20 GB per 10 k reads for 2.5 GB of cells); the strand flip of a backward cell keeps its node's four table values while the
		// node stays the same.
		constexpr uint32_t PATH_REGS = 6;
		uint32_t pn0 = 0, pn1 = 0, pn2 = 0, pn3 = 0, pn4 = 0, pn5 = 0;
		uint32_t pathLen = 0, last = 0xffffffffu;
		AnchorRec rec;
		rec.firstNode = rec.firstOffset = rec.firstSeqPos = 0;
		rec.lastNode = rec.lastOffset = rec.lastSeqPos = 0;
		bool haveFirst = false;
		auto visit = [&](uint32_t node, uint32_t off, int32_t sp) __attribute__((always_inline)) {
			if (node != last) {
				switch (pathLen) { case 0: pn0 = node; break; case 1: pn1 = node; break; case 2: pn2 = node; break; case 3: pn3 = node; break; case 4: pn4 = node; break; case 5: pn5 = node; break; default: break; }
				pathLen++; last = node;
			}
			if (!haveFirst) { rec.firstNode = node; rec.firstOffset = off; rec.firstSeqPos = (uint32_t)sp; haveFirst = true; }
			rec.lastNode = node; rec.lastOffset = off; rec.lastSeqPos = (uint32_t)sp;
		};
		{
			uint32_t cachedNode = 0xffffffffu, nodeOff = 0, origSz = 0, lookupBase = 0, cachedBlock = 0xffffffffu, twin = 0, twinBase = 0;
			for (uint32_t i0 = 0; i0 < v.nBw; i0 += 8) {
				PoolCell c[8];
#pragma unroll
				for (uint32_t u = 0; u < 8; u++) c[u] = v.bw[min(i0 + u, v.nBw - 1)];
#pragma unroll
				for (uint32_t u = 0; u < 8; u++) {
					if (i0 + u >= v.nBw) break;
					if (c[u].node != cachedNode) {
						cachedNode = c[u].node;
						const int32_t id = g.nodeIDs[cachedNode];
						nodeOff = g.nodeOffset[cachedNode]; origSz = g.origSize[id]; lookupBase = g.lookupOff[id ^ 1];
						cachedBlock = 0xffffffffu;
					}
					const uint32_t rev = origSz - 1 - (nodeOff + (c[u].offsetAndSwitch & 255u));   // GetReversePosition + GetUnitigNode, as in mergedCell
					if (rev / 64 != cachedBlock) { cachedBlock = rev / 64; twin = g.lookup[lookupBase + cachedBlock]; twinBase = g.nodeOffset[twin]; }
					visit(twin, rev - twinBase, v.p - 1 - c[u].seqPos);
				}
			}
			for (uint32_t i0 = 0; i0 < v.nFw; i0 += 8) {   // the forward trace runs towards the seed: used back to front
				PoolCell c[8];
#pragma unroll
				for (uint32_t u = 0; u < 8; u++) c[u] = v.fw[v.nFw - 1 - min(i0 + u, v.nFw - 1)];
#pragma unroll
				for (uint32_t u = 0; u < 8; u++) {
					if (i0 + u >= v.nFw) break;
					visit(c[u].node, c[u].offsetAndSwitch & 255u, v.p + 1 + c[u].seqPos);
				}
			}
		}
		unsigned long long base = atomicAdd(pathCursor, (unsigned long long)pathLen);
		if (base + pathLen > pathCapacity) { status = 2; break; }
		rec.valid = 1;
		rec.x = fr.l;
		rec.y = fr.l + (uint32_t)splitLen - 1;
		rec.pad = 0;
		rec.pathOff = base;
		rec.pathLen = pathLen;
		rec.score = (hasB ? eb.score : 0) + (hasF ? ef.score : 0);
		if (pathLen <= PATH_REGS) {
			if (pathLen > 0) pathPool[base] = pn0;
			if (pathLen > 1) pathPool[base + 1] = pn1;
			if (pathLen > 2) pathPool[base + 2] = pn2;
			if (pathLen > 3) pathPool[base + 3] = pn3;
			if (pathLen > 4) pathPool[base + 4] = pn4;
			if (pathLen > 5) pathPool[base + 5] = pn5;
		} else {
			uint32_t w = 0;
			last = 0xffffffffu;
			for (uint32_t i = 0; i < n; i++) {
				uint32_t node, off; int32_t sp;
				mergedCell(g, v, i, node, off, sp);
				if (node != last) { pathPool[base + w++] = node; last = node; }
			}
		}
		anchors[sIdx] = rec;
	}
	if (status != 0) for (uint32_t k = 0; k < nSeeds; k++) anchors[fr.seedBegin + k].valid = 0;   // a throwing AlignOneWay returns nothing
	fragStatus[f] = status;
	fragExtended[f] = extended;
}

// Work items of the fragment pass, built where they are used (src/GraphAligner.h:499-511 per seed of a fragment window): the seed glue sorts each
// read's seeds and cuts the windows (order-critical, gc_seedglue.hip) and leaves 16 B per fragment and per seed; one thread per fragment
// expands its seed window into the per-slot records - the seed in fragment order and the two extensions (backward: reverse complement of the
// fragment's prefix from the seed's reverse-strand twin; forward: the suffix from the seed). On the host this was 70 ms per 10 k reads
// (345 MB of records through pinned memory, a twin lookup per slot) on the fragment pipeline's critical path, plus the upload.
__global__ void __launch_bounds__(256) k_build_fragment_work(DGraph g, const Fragment* __restrict__ frags, const uint32_t* __restrict__ fragFirstSeed, uint32_t nFrags,
	const FragSeed* __restrict__ readSeeds, const uint64_t* __restrict__ readOffsets, uint64_t totalBases, uint32_t splitLen, FragSeed* __restrict__ fragSeeds, ExtItem* __restrict__ work,
	ExtResult* __restrict__ results)
{
	const uint32_t F = blockIdx.x * 256 + threadIdx.x;
	if (F >= nFrags) return;
	const Fragment fr = frags[F];
	const uint64_t readOff = readOffsets[fr.read], len = readOffsets[fr.read + 1] - readOff;
	const FragSeed* seeds = readSeeds + fragFirstSeed[F];
	for (uint32_t k = 0; k < fr.seedEnd - fr.seedBegin; k++) {
		const FragSeed s = seeds[k];
		const uint32_t slot = fr.seedBegin + k, p = s.seqPos - fr.l;
		fragSeeds[slot] = s;
		ExtItem b;
		b.seqOff = totalBases + readOff + (len - fr.l - p);
		b.seqLen = p;
		twinOf(g, s.node, s.offset, b.node, b.offset);
		b.pad = fr.read;
		ExtItem f;
		f.seqOff = readOff + fr.l + p + 1;
		f.seqLen = splitLen - 1 - p;
		f.node = s.node;
		f.offset = s.offset;
		f.pad = fr.read;
		work[2 * (size_t)slot] = b;
		work[2 * (size_t)slot + 1] = f;
		if (results) {   // lazy extension: nothing has run yet
			results[2 * (size_t)slot] = ExtResult { 0, 0, EXT_NOT_RUN, 0, 0 };
			results[2 * (size_t)slot + 1] = ExtResult { 0, 0, EXT_NOT_RUN, 0, 0 };
		}
	}
}

// =====================================================================================================
// launchers
// =====================================================================================================

void launchBuildAnchors(hipStream_t stream, const DGraph& g, const Fragment* frags, uint32_t nFrags, const FragSeed* seeds, const ExtResult* ext,
	const PoolCell* tracePool, int32_t splitLen, AnchorRec* anchors, uint32_t* fragStatus, uint32_t* fragExtended,
	uint32_t* pathPool, unsigned long long* pathCursor, uint64_t pathCapacity, AnchorRounds rounds, uint32_t* readTies)
{
	if (nFrags == 0) return;
	hipLaunchKernelGGL(k_build_anchors, dim3((nFrags + 63) / 64), dim3(64), 0, stream, g, frags, nFrags, seeds, ext, tracePool, splitLen, anchors, fragStatus, fragExtended, pathPool, pathCursor, pathCapacity, rounds, readTies);
}

void launchBuildFragmentWork(hipStream_t stream, const DGraph& g, const Fragment* frags, const uint32_t* fragFirstSeed, uint32_t nFrags, const FragSeed* readSeeds, const uint64_t* readOffsets,
	uint64_t totalBases, uint32_t splitLen, FragSeed* fragSeeds, ExtItem* work, ExtResult* results)
{
	if (nFrags) hipLaunchKernelGGL(k_build_fragment_work, dim3((nFrags + 255) / 256), dim3(256), 0, stream, g, frags, fragFirstSeed, nFrags, readSeeds, readOffsets, totalBases, splitLen, fragSeeds, work, results);
}

} // namespace gcdev
