// The whole-read pass (K3-long) apart from its extension kernel (gc_long_extend.hpp): the per-read rules of AlignOneWay, the round kernels around the
// extension launches, and the one-lane-per-read fallback kernel that shares those rules.
#include "gc_kernels.hpp"
#include "gc_device_wave.hpp"   // unpackCell: the extension kernel's packed trace cells

namespace gcdev {

// =====================================================================================================
// K3-long - the whole-read GraphAligner pass. reference: AlignOneWay with sloppyOptimizations,
// src/GraphAligner.h:114-203 (called from src/Aligner.cpp:565), getAlignmentFromSeed :567-626,
// exactAlignmentPart :407-461. The reference walks a read's seeds in goodness order and every decision
// (skip because an earlier alignment covers the seed, stop because the read is aligned end to end)
// depends on the alignments produced so far, so a read is one sequential unit: one lane per read, the
// multi-slice extension core of gc_device.hpp does the work. All reads of a batch have similar length,
// which keeps the lanes of a wave in step at slice granularity.
// =====================================================================================================

struct LongSlab { LaneScratch sc; TraceCell* traceB; };   // backward trace is parked while the forward extension reuses sc.trace

__device__ __forceinline__ LongSlab longSlab(uint8_t* slab, const ExtendConfig& cfg)
{
	LongSlab ls;
	ls.sc = laneScratch(slab, cfg);
	ls.traceB = (TraceCell*)(ls.sc.itemNodes + cfg.maxItems);   // (behind the lane's extension slab)
	return ls;
}

// Is the seed's cell on this alignment's trace? (:407-461). Returns 1 yes, 0 no, 2 the reference asserts.
__device__ inline int onTrace(const LongCell* trace, uint32_t n, uint32_t seqPos, int32_t compareNode, uint32_t nodeOffset)
{
	if (!(trace[n - 1].seqPos > trace[0].seqPos)) return 2;
	if (trace[n - 1].seqPos < seqPos || trace[0].seqPos > seqPos) return 0;
	uint32_t lo = 0, hi = n;   // first cell with seqPos >= target (seqPos is non-decreasing along the trace)
	while (lo < hi) {
		uint32_t mid = (lo + hi) / 2;
		if (trace[mid].seqPos < seqPos) lo = mid + 1; else hi = mid;
	}
	for (uint32_t i = lo; i < n && trace[i].seqPos == seqPos; i++)
		if (trace[i].node == compareNode && trace[i].offset == nodeOffset) return 1;
	return 0;
}

// seedScoreForEndToEndAln update after an alignment was added. reference: src/GraphAligner.h:181-198 - the list is
// sorted by alignmentStart; if the first starts at 0, later alignments whose start is <= the running end extend it;
// if the union reaches the read's end the minimum seedGoodness of the contributing alignments becomes the cut-off.
// Visiting in ascending start makes the outcome independent of the order among equal starts, so no sort is needed.
// The two rules that end AlignOneWay's scan (src/GraphAligner.h:127,132), on the state as it stands before the seed. extraHeuristic: gc_params::extra_heuristic
// (nondeterministicOptimizations); extendSeeds: the read's seed budget (LongJob::extendSeeds).
__device__ __forceinline__ bool seedCutEndToEnd(uint32_t goodness, uint32_t e2eScore, uint32_t extraHeuristic)
{
	return goodness < e2eScore || (extraHeuristic && goodness == e2eScore);
}
__device__ __forceinline__ bool seedCutBudget(uint32_t goodness, uint32_t extended, uint32_t extendSeeds, uint32_t worstExtended, uint32_t extraHeuristic)
{
	return extended >= extendSeeds && (extraHeuristic || goodness < worstExtended);
}

__device__ inline uint32_t endToEndScore(LongAln* mine, uint32_t nAln, uint32_t readLen, uint32_t current)
{
	bool anyAtZero = false;
	for (uint32_t a = 0; a < nAln; a++) if (mine[a].start == 0) anyAtZero = true;
	if (!anyAtZero) return current;
	uint32_t contiguousEnd = 0, minGoodness = 0xffffffffu;
	bool first = true;
	for (uint32_t visited = 0; visited < nAln; visited++) {
		uint32_t best = 0xffffffffu;
		for (uint32_t a = 0; a < nAln; a++) {
			if (mine[a].pad) continue;
			if (best == 0xffffffffu || mine[a].start < mine[best].start) best = a;
		}
		mine[best].pad = 1;
		if (first) { contiguousEnd = mine[best].end; minGoodness = mine[best].goodness; first = false; continue; }
		if (mine[best].start <= contiguousEnd) {
			minGoodness = mine[best].goodness < minGoodness ? mine[best].goodness : minGoodness;
			contiguousEnd = mine[best].end > contiguousEnd ? mine[best].end : contiguousEnd;
		}
	}
	for (uint32_t a = 0; a < nAln; a++) mine[a].pad = 0;
	return contiguousEnd == readLen ? minGoodness : current;
}

template <bool BAND, bool CLIP = false>   // BAND: the band controls of cfg (extendSeedT<.., true>); CLIP: precise clipping / the X-drop (extendSeedT<.., true, true>)
__global__ void __launch_bounds__(64) k_long_pass(DGraph g, const CorrectnessTables* __restrict__ ct, const uint8_t* __restrict__ iupac, ExtendConfig cfg,
	const LongJob* __restrict__ jobs, uint32_t nReads, const LongSeed* __restrict__ seeds, const char* __restrict__ bases, uint64_t rcBase,
	uint32_t minClusterSize, uint32_t extraHeuristic, uint8_t* __restrict__ scratch, uint64_t slabBytes,
	LongCell* __restrict__ cellPool, unsigned long long* __restrict__ cellCursor, uint64_t cellCapacity,
	LongAln* __restrict__ alns, LongReadResult* __restrict__ results, unsigned long long* __restrict__ counters)
{
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t stride = gridDim.x * blockDim.x;
	LongSlab ls = longSlab(scratch + (uint64_t)tid * slabBytes, cfg);
	ExtCounters cnt {};
	for (uint32_t r = tid; r < nReads; r += stride) {
		LongJob job = jobs[r];
		LongAln* mine = alns + job.alnBegin;
		uint32_t nAln = 0, extended = 0, status = 0, ties = 0;
		uint32_t e2eScore = 0;   // seedScoreForEndToEndAln
		uint32_t worstExtended = 0;   // worstExtendedSeedScore
		const int L = (int)job.readLen;
		// Lanes of a wave must reach the expensive part (the extension) together: a plain loop over seeds would let
		// every lane extend at a different iteration and serialise the wave's extensions. So each lane first advances
		// to its next seed that needs extending (cheap, divergent), then all lanes that found one extend in step.
		uint32_t si = job.seedBegin;
		while (true) {
			bool have = false;
			LongSeed sd {};
			for (; status == 0 && si < job.seedEnd && !have; si++) {
				sd = seeds[si];
				if (seedCutEndToEnd(sd.goodness, e2eScore, extraHeuristic)) { si = job.seedEnd; break; }   // aligned end to end, skip the rest (:127-131)
				if (seedCutBudget(sd.goodness, extended, job.extendSeeds, worstExtended, extraHeuristic)) { si = job.seedEnd; break; }   // enough seeds extended (:132-136)
				if (sd.clusterSize < minClusterSize) continue;              // :141-146
				bool skip = false;
				for (uint32_t a = 0; a < nAln; a++)                          // sloppy overlap rule (:147-161)
					if (mine[a].start <= sd.seqPos && mine[a].end >= sd.seqPos && (extraHeuristic || mine[a].goodness > sd.goodness)) { skip = true; break; }
				if (skip) continue;
				int32_t compareNode = g.nodeIDs[sd.node];
				uint32_t compareOffset = g.nodeOffset[sd.node] + sd.offset;
				for (uint32_t a = 0; a < nAln && !skip; a++) {              // exactAlignmentPart (:163-173)
					int on = onTrace(cellPool + mine[a].traceOff, mine[a].traceLen, sd.seqPos, compareNode, compareOffset);
					if (on == 2) { status = 1; break; }
					if (on == 1) skip = true;
				}
				if (skip || status) continue;
				have = true;
			}
			if (!__any(have)) break;
			if (!have) continue;
			worstExtended = sd.goodness;   // :175-176, failed extensions included
			extended++;
			// getAlignmentFromSeed (:567-626): backward on revcomp(read[0..p)), forward on read(p..]
			const int p = (int)sd.seqPos;
			uint32_t nB = 0, nF = 0;
			int32_t scoreB = 0, scoreF = 0;
			uint32_t stB = EXT_FAILED, stF = EXT_FAILED;
			if (p > 0) {
				uint32_t twinNode, twinOffset;
				twinOf(g, sd.node, sd.offset, twinNode, twinOffset);
				stB = extendSeed<BAND, CLIP>(g, *ct, iupac, cfg, ls.sc, bases + rcBase + job.readOff + (uint64_t)(L - p), p, twinNode, twinOffset, nB, scoreB, cnt);
				ties += cnt.flattenTie;
				if (stB == EXT_OK) for (uint32_t i = 0; i < nB; i++) ls.traceB[i] = ls.sc.trace[i];
			}
			if (p < L - 1 && stB != EXT_ASSERT) { stF = extendSeed<BAND, CLIP>(g, *ct, iupac, cfg, ls.sc, bases + job.readOff + (uint64_t)(p + 1), L - 1 - p, sd.node, sd.offset, nF, scoreF, cnt); ties += cnt.flattenTie; }   // (a throwing backward extension ends getAlignmentFromSeed before the forward one runs)
			if (stB == EXT_ASSERT || stF == EXT_ASSERT) { status = 1; break; }
			if (stB == EXT_OVERFLOW || stF == EXT_OVERFLOW) { status = 2; break; }
			bool hasB = stB == EXT_OK, hasF = stF == EXT_OK;
			if (!hasB && !hasF) continue;   // alignmentFailed()
			if (nAln >= job.alnCap) { status = 3; break; }
			uint32_t useB = hasB ? (hasF ? nB - 1 : nB) : 0;
			uint32_t total = useB + (hasF ? nF : 0);
			unsigned long long base = atomicAdd(cellCursor, (unsigned long long)total);
			if (base + total > cellCapacity) { status = 4; break; }
			LongCell* outCells = cellPool + base;
			for (uint32_t i = 0; i < useB; i++) {   // fixReverseTraceSeqPosAndOrder (:543-565)
				const TraceCell& c = ls.traceB[i];
				uint32_t off = c.offsetAndSwitch & 255u;
				int32_t id = g.nodeIDs[c.node];
				uint32_t orig = g.nodeOffset[c.node] + off;
				LongCell oc;
				oc.node = id ^ 1;
				oc.offset = g.origSize[id] - 1 - orig;
				oc.seqPos = (uint32_t)(p - 1 - c.seqPos);
				oc.nodeSwitch = (i + 1 < nB) ? ((ls.traceB[i + 1].offsetAndSwitch >> 8) & 1u) : 0u;
				outCells[i] = oc;
			}
			if (hasF) for (uint32_t i = 0; i < nF; i++) {   // fixForwardTraceSeqPos (:527-540), device order reversed
				const TraceCell& c = ls.sc.trace[nF - 1 - i];
				LongCell oc;
				oc.node = g.nodeIDs[c.node];
				oc.offset = g.nodeOffset[c.node] + (c.offsetAndSwitch & 255u);
				oc.seqPos = (uint32_t)(p + 1 + c.seqPos);
				oc.nodeSwitch = (c.offsetAndSwitch >> 8) & 1u;
				outCells[useB + i] = oc;
			}
			LongAln al;
			al.start = outCells[0].seqPos;
			al.end = outCells[total - 1].seqPos + 1;
			al.score = (uint32_t)((hasB ? scoreB : 0) + (hasF ? scoreF : 0));
			al.goodness = sd.goodness;
			al.traceOff = base;
			al.traceLen = total;
			al.pad = 0;
			mine[nAln++] = al;
			e2eScore = endToEndScore(mine, nAln, (uint32_t)L, e2eScore);
		}
		LongReadResult rr;
		rr.nAlignments = status == 1 ? 0 : nAln;   // a throwing AlignOneWay returns nothing (src/Aligner.cpp:585-592)
		rr.seedsExtended = extended;
		rr.status = status;
		rr.pad = ties;
		results[r] = rr;
	}
	if (cnt.extensions) {
		atomicAdd(&counters[0], cnt.dpTiles);
		atomicAdd(&counters[1], cnt.recomputeTiles);
		atomicAdd(&counters[2], cnt.columnSteps);
		atomicAdd(&counters[3], cnt.traceItems);
		atomicAdd(&counters[4], cnt.extensions);
		atomicAdd(&counters[5], cnt.backtraceTiles);
	}
}

// =====================================================================================================
// K3-long in rounds. The monolithic kernel above keeps a lane busy for as many rounds as its read needs while the
// other 63 lanes of the wave wait (3.6 seeds are extended per read on average, up to 10). Here every round is
//   select  - one wave per read: the reference's skip rules for 64 seeds at once, then its in-order scan on the ballot
//             masks; emits two work items (backward, forward) per chosen seed;
//   extend  - one wave per work item (k_long_extend<1>), longest first; the trace goes to a pool;
//   merge   - one wave per read: joins the two traces 64 cells at a time, appends the alignment, updates the cut-off;
// and the host launches rounds until no read emits work. Results are identical to the monolithic kernels.
// =====================================================================================================

__global__ void __launch_bounds__(256) k_long_init(const LongJob* __restrict__ jobs, uint32_t nReads, LongState* __restrict__ state)
{
	GC_RAISE_PRIO();
	uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= nReads) return;
	LongState st { jobs[r].seedBegin, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	state[r] = st;
}

// Skip rules of AlignOneWay for one seed against alignments [aFrom, aTo) of the read (:147-173).
// Returns 0 extend, 1 skip, 2 the reference asserts.
__device__ inline int seedSkipped(const DGraph& g, const LongSeed& sd, const LongAln* mine, uint32_t aFrom, uint32_t aTo, const LongCell* cellPool, uint32_t extraHeuristic)
{
	for (uint32_t a = aFrom; a < aTo; a++)                          // sloppy overlap rule (:147-161; with extra_heuristic whatever the goodness, :152)
		if (mine[a].start <= sd.seqPos && mine[a].end >= sd.seqPos && (extraHeuristic || mine[a].goodness > sd.goodness)) return 1;
	int32_t compareNode = g.nodeIDs[sd.node];
	uint32_t compareOffset = g.nodeOffset[sd.node] + sd.offset;
	for (uint32_t a = aFrom; a < aTo; a++) {                        // exactAlignmentPart (:163-173)
		int on = onTrace(cellPool + mine[a].traceOff, mine[a].traceLen, sd.seqPos, compareNode, compareOffset);
		if (on == 2) return 2;
		if (on == 1) return 1;
	}
	return 0;
}

// One wave per read: advance to the next seed(s) that need extending and emit their work items. The skip rules of 64
// seeds are evaluated at once (each is a chain of dependent loads: a binary search in every alignment's trace), then
// the reference's in-order scan is replayed on the ballot masks. With maxCandidates > 1 (used for the tail rounds,
// when few reads are still active and the chip is idle) further seeds are emitted speculatively: they pass the skip
// rules against the alignments known now; k_long_merge re-checks each of them against the alignments added before it
// in the same round, so the outcome equals one-seed-per-round.
// The two rules that end the scan are ballots on the state the last merge committed: seeds come in falling goodness, so a seed they cut stays cut
// whatever the candidates in front of it become. The seed budget counts extensions, and the merge may skip a pending candidate, so on the PENDING
// count the scan only stops emitting (si stays on the seed; the next round sees it with the committed count) - it never ends there.
#define LONG_MAX_CANDIDATES 8
__device__ __forceinline__ void longSelectRead(const DGraph& g, const uint32_t r, const uint32_t lane, const LongJob* __restrict__ jobs, const LongSeed* __restrict__ seeds, uint32_t minClusterSize,
	uint32_t extraHeuristic, uint32_t maxCandidates, LongState* __restrict__ state, const LongAln* __restrict__ alns, const LongCell* __restrict__ cellPool, LongWork* __restrict__ work, uint32_t* __restrict__ workLen, uint32_t* __restrict__ candSeed,
	unsigned long long* __restrict__ workCount, uint64_t workCapacity)
{
	LongState st = state[r];
	st.candCount = 0;
	if (st.status != 0) { if (lane == 0) state[r] = st; return; }
	LongJob job = jobs[r];
	const LongAln* mine = alns + job.alnBegin;
	uint32_t cand[LONG_MAX_CANDIDATES];
	uint32_t nCand = 0;
	uint32_t si = st.si;
	bool stop = false;
	while (!stop && si < job.seedEnd) {
		const uint32_t idx = si + lane;
		const bool valid = idx < job.seedEnd;
		LongSeed sd = seeds[valid ? idx : si];
		const bool cut = valid && (seedCutEndToEnd(sd.goodness, st.e2eScore, extraHeuristic)                                       // aligned end to end (:127-131)
			|| seedCutBudget(sd.goodness, st.extended, job.extendSeeds, st.worstExtended, extraHeuristic));                          // enough seeds extended (:132-136)
		const bool small = sd.clusterSize < minClusterSize;                       // :141-146
		int sk = 1;
		if (valid && !cut && !small) sk = seedSkipped(g, sd, mine, 0, st.nAln, cellPool, extraHeuristic);
		const uint64_t cutMask = __ballot(cut), assertMask = __ballot(sk == 2), candMask = __ballot(sk == 0);
		const uint32_t nValid = job.seedEnd - si < 64 ? job.seedEnd - si : 64;
		const uint32_t firstCut = cutMask ? (uint32_t)__ffsll((unsigned long long)cutMask) - 1 : 64;
		const uint32_t limit = firstCut < nValid ? firstCut : nValid;
		uint32_t b = 0;
		for (; b < limit; b++) {   // the reference's scan, in seed order (uniform across the wave)
			if ((assertMask >> b) & 1) { st.status = 1; stop = true; break; }
			if ((candMask >> b) & 1) {
				if (nCand > 0 && st.extended + nCand >= job.extendSeeds) { stop = true; break; }   // the pending candidates may fill the budget: no more this round
				for (uint32_t k = 0; k < LONG_MAX_CANDIDATES; k++) if (k == nCand) cand[k] = si + b;
				nCand++;
				if (nCand == maxCandidates) { b++; stop = true; break; }
			}
		}
		si += b;
		if (!stop && firstCut < nValid) { si = job.seedEnd; stop = true; }
	}
	st.si = si;
	if (nCand > 0) {
		unsigned long long at = 0;
		if (lane == 0) at = atomicAdd(workCount, 2ull * nCand);
		at = __shfl(at, 0);
		if (at + 2ull * nCand > workCapacity) { st.status = 2; nCand = 0; }
		st.candBegin = (uint32_t)(at / 2);
		st.candCount = nCand;
		uint32_t myCand = 0;
		for (uint32_t k = 0; k < LONG_MAX_CANDIDATES; k++) if (k == lane) myCand = cand[k];
		if (lane < nCand) {
			const uint32_t c = lane;
			LongSeed sd = seeds[myCand];
			const uint32_t L = job.readLen, p = sd.seqPos;
			// backward: rows are revcomp(read[0..p)) = reverse-complement strand from position L-p; forward: read(p..] from p+1
			uint32_t twinNode, twinOffset;
			twinOf(g, sd.node, sd.offset, twinNode, twinOffset);
			work[at + 2 * c] = LongWork { job.maskOff + 4ull * job.maskWords, job.maskWords, L - p, p, twinNode, twinOffset, r };
			work[at + 2 * c + 1] = LongWork { job.maskOff, job.maskWords, p + 1, L - 1 - p, sd.node, sd.offset, r };
			workLen[at + 2 * c] = p;
			workLen[at + 2 * c + 1] = L - 1 - p;
			candSeed[at / 2 + c] = myCand;
		}
	}
	if (lane == 0) state[r] = st;
}
__global__ void __launch_bounds__(64) k_long_select(DGraph g, const LongJob* __restrict__ jobs, uint32_t nReads, const LongSeed* __restrict__ seeds, uint64_t rcBase, uint32_t minClusterSize,
	uint32_t extraHeuristic, uint32_t maxCandidates, LongState* __restrict__ state, const LongAln* __restrict__ alns, const LongCell* __restrict__ cellPool, LongWork* __restrict__ work, uint32_t* __restrict__ workLen, uint32_t* __restrict__ candSeed,
	unsigned long long* __restrict__ workCount, uint64_t workCapacity)
{
	GC_RAISE_PRIO();
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= nReads) return;
	longSelectRead(g, r, lane, jobs, seeds, minClusterSize, extraHeuristic, maxCandidates, state, alns, cellPool, work, workLen, candSeed, workCount, workCapacity);
}

// One wave per read: the decisions are taken redundantly by all lanes (uniform control flow, lane 0 does the single
// writes), the trace -> cell conversion - the bulk of the work, ~1.5 cells per read base - runs 64 cells at a time.
__device__ __forceinline__ void longMergeRead(const DGraph& g, const uint32_t r, const uint32_t lane, const LongJob* __restrict__ jobs, const LongSeed* __restrict__ seeds, const uint32_t* __restrict__ candSeed,
	const LongWorkResult* __restrict__ results, const unsigned long long* __restrict__ tracePool,
	LongState* state, LongAln* alns, LongCell* cellPool, unsigned long long* __restrict__ cellCursor, uint64_t cellCapacity, uint32_t extraHeuristic)
{
	LongState st = state[r];
	if (st.candCount == 0 || st.status != 0) return;
	LongJob job = jobs[r];
	LongAln* mine = alns + job.alnBegin;
	const int L = (int)job.readLen;
	const uint32_t nAlnAtSelect = st.nAln;
	for (uint32_t c = 0; c < st.candCount && st.status == 0; c++) {
		const uint32_t pair = st.candBegin + c;
		const uint32_t seedIdx = candSeed[pair];
		LongSeed sd = seeds[seedIdx];
		if (c > 0) {
			// re-check against what this round added before this candidate (the select kernel checked the older alignments)
			// (:127 and :132 first, on the state the candidates before this one have left)
			if (seedCutEndToEnd(sd.goodness, st.e2eScore, extraHeuristic)) { st.si = job.seedEnd; break; }
			if (seedCutBudget(sd.goodness, st.extended, job.extendSeeds, st.worstExtended, extraHeuristic)) { st.si = job.seedEnd; break; }
			int sk = seedSkipped(g, sd, mine, nAlnAtSelect, st.nAln, cellPool, extraHeuristic);
			if (sk == 2) { st.status = 1; break; }
			if (sk == 1) continue;
		}
		st.worstExtended = sd.goodness;   // :175-176, failed extensions included
		st.extended++;
		const LongWorkResult rb = results[2 * pair], rf = results[2 * pair + 1];
		const int p = (int)sd.seqPos;
		bool runB = p > 0, runF = p < L - 1;
		uint32_t stB = runB ? rb.status : EXT_FAILED, stF = runF ? rf.status : EXT_FAILED;
		if (runB) st.pad1 += rb.pad & 1u;                                              // LongState::pad1 = the read's flatten ties (gc_result::flatten_ties_long)
		if (runF && stB != EXT_ASSERT) st.pad1 += rf.pad & 1u;                         // (the forward extension only runs when the backward one did not throw)
		if (stB == EXT_ASSERT || stF == EXT_ASSERT) { st.status = 1; break; }          // getAlignmentFromSeed threw
		if (stB == EXT_OVERFLOW || stF == EXT_OVERFLOW) { st.status = 2; break; }
		if (stB == EXT_LDS_CAP || stF == EXT_LDS_CAP) { st.status = 5; break; }
		bool hasB = stB == EXT_OK, hasF = stF == EXT_OK;
		if (!hasB && !hasF) continue;   // alignmentFailed()
		uint32_t nB = rb.traceLen, nF = rf.traceLen;
		uint32_t useB = hasB ? (hasF ? nB - 1 : nB) : 0;
		uint32_t total = useB + (hasF ? nF : 0);
		if (st.nAln >= job.alnCap) { st.status = 3; break; }
		unsigned long long base = 0;
		if (lane == 0) base = atomicAdd(cellCursor, (unsigned long long)total);
		base = __shfl(base, 0);
		if (base + total > cellCapacity) { st.status = 4; break; }
		LongCell* outCells = cellPool + base;
		for (uint32_t i = lane; i < useB; i += 64) {   // fixReverseTraceSeqPosAndOrder (:543-565)
			TraceCell tc = unpackCell(tracePool[rb.traceOff + i]);
			uint32_t off = tc.offsetAndSwitch & 255u;
			int32_t id = g.nodeIDs[tc.node];
			uint32_t orig = g.nodeOffset[tc.node] + off;
			LongCell oc;
			oc.node = id ^ 1;
			oc.offset = g.origSize[id] - 1 - orig;
			oc.seqPos = (uint32_t)(p - 1 - tc.seqPos);
			oc.nodeSwitch = (i + 1 < nB) ? ((unpackCell(tracePool[rb.traceOff + i + 1]).offsetAndSwitch >> 8) & 1u) : 0u;
			outCells[i] = oc;
		}
		if (hasF) for (uint32_t i = lane; i < nF; i += 64) {   // fixForwardTraceSeqPos (:527-540), device order reversed
			TraceCell tc = unpackCell(tracePool[rf.traceOff + (nF - 1 - i)]);
			LongCell oc;
			oc.node = g.nodeIDs[tc.node];
			oc.offset = g.nodeOffset[tc.node] + (tc.offsetAndSwitch & 255u);
			oc.seqPos = (uint32_t)(p + 1 + tc.seqPos);
			oc.nodeSwitch = (tc.offsetAndSwitch >> 8) & 1u;
			outCells[useB + i] = oc;
		}
		__threadfence_block();   // the cells are read back below and by the next candidate's skip rules (one wave per read: the fence orders its own stores and loads)
		LongAln al;
		al.start = outCells[0].seqPos;
		al.end = outCells[total - 1].seqPos + 1;
		al.score = (uint32_t)((hasB ? rb.score : 0) + (hasF ? rf.score : 0));
		al.goodness = sd.goodness;
		al.traceOff = base;
		al.traceLen = total;
		al.pad = 0;
		uint32_t e2e = 0;
		if (lane == 0) {
			mine[st.nAln] = al;
			e2e = endToEndScore(mine, st.nAln + 1, (uint32_t)L, st.e2eScore);
		}
		st.nAln++;
		st.e2eScore = __shfl(e2e, 0);
		__threadfence_block();
	}
	st.candCount = 0;
	if (lane == 0) state[r] = st;
}

__global__ void __launch_bounds__(64) k_long_merge(DGraph g, const LongJob* __restrict__ jobs, uint32_t nReads, const LongSeed* __restrict__ seeds, const uint32_t* __restrict__ candSeed,
	const LongWorkResult* __restrict__ results, const unsigned long long* __restrict__ tracePool,
	LongState* state, LongAln* alns, LongCell* cellPool, unsigned long long* __restrict__ cellCursor, uint64_t cellCapacity, uint32_t extraHeuristic)
{
	GC_RAISE_PRIO();
	const uint32_t r = blockIdx.x;
	if (r >= nReads) return;
	longMergeRead(g, r, threadIdx.x, jobs, seeds, candSeed, results, tracePool, state, alns, cellPool, cellCursor, cellCapacity, extraHeuristic);
}

// Execution order of a round's work items: longest extensions first (a counting sort over 1024 length classes, one block;
// the order inside a class is whatever the atomics give - results do not depend on it). mode 0: identity.
#ifndef GC_ORDER_THREADS
#define GC_ORDER_THREADS 256    // threads of the ordering block (r5: 256 - under config 5 the 1 024-thread block waited up to 150 ms per round for sixteen free wave slots on one CU, with the whole-read token held; r4 note: (-DGC_ORDER_THREADS=256: a wave scan of the histogram and a block that finds its wave slots sooner among five batches' kernels - measured, 147.8 / 151.7 / 150.5 ms per batch against 150.8 / 150.2 / 149.8, `gpurun_out/r4_ord`: no effect)
#endif
__global__ void __launch_bounds__(GC_ORDER_THREADS) k_long_order(const uint32_t* __restrict__ workLen, const unsigned long long* __restrict__ workCount, uint32_t* __restrict__ order, uint32_t shift, uint32_t mode)
{
	GC_RAISE_PRIO();
	__shared__ uint32_t hist[1024];
	__shared__ uint32_t start[1024];
	const uint32_t n = (uint32_t)*workCount, tid = threadIdx.x, T = GC_ORDER_THREADS;
	if (mode == 0) { for (uint32_t i = tid; i < n; i += T) order[i] = i; return; }
	for (uint32_t b = tid; b < 1024; b += T) hist[b] = 0;
	__syncthreads();
	for (uint32_t i = tid; i < n; i += T) { uint32_t b = workLen[i] >> shift; atomicAdd(&hist[1023 - (b < 1023 ? b : 1023)], 1u); }
	__syncthreads();
#if GC_ORDER_THREADS == 1024
	if (tid == 0) { uint32_t at = 0; for (uint32_t b = 0; b < 1024; b++) { start[b] = at; at += hist[b]; } }
#else
	if (tid < 64) {   // the first wave: sixteen classes per lane, a wave scan of the lanes' sums
		uint32_t mine[16], sum = 0;
		for (uint32_t k = 0; k < 16; k++) { mine[k] = hist[tid * 16 + k]; sum += mine[k]; }
		uint32_t incl = sum;
		for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d); if ((int)tid >= d) incl += o; }
		uint32_t at = incl - sum;
		for (uint32_t k = 0; k < 16; k++) { start[tid * 16 + k] = at; at += mine[k]; }
	}
#endif
	__syncthreads();
	for (uint32_t i = tid; i < n; i += T) { uint32_t b = workLen[i] >> shift; order[atomicAdd(&start[1023 - (b < 1023 ? b : 1023)], 1u)] = i; }
}

// copies a few cursor words into pinned host memory through the compute queue (a copy-engine transfer would queue behind bulk uploads)
__global__ void k_publish(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, uint32_t nWords)
{
	GC_RAISE_PRIO();
	if (threadIdx.x < nWords) { dst[threadIdx.x] = src[threadIdx.x]; __threadfence_system(); }
}

// a few words set to zero by a kernel: a hipMemsetAsync inside the round loop may go through a copy engine and queue behind another
// batch's bulk uploads
__global__ void k_zero_words(unsigned long long* __restrict__ dst, uint32_t nWords)
{
	GC_RAISE_PRIO();
	if (threadIdx.x < nWords) dst[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) k_long_finish(uint32_t nReads, const LongState* __restrict__ state, LongReadResult* __restrict__ results)
{
	GC_RAISE_PRIO();
	uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= nReads) return;
	LongState st = state[r];
	LongReadResult rr { st.status == 1 ? 0u : st.nAln, st.extended, st.status, st.pad1 };   // pad = the read's flatten ties   // a throwing AlignOneWay returns nothing (src/Aligner.cpp:585-592)
	results[r] = rr;
}

// =====================================================================================================
// launchers
// =====================================================================================================

uint64_t longSlabBytes(const ExtendConfig& cfg) { return (extendSlabBytes(cfg) + sizeof(TraceCell) * (uint64_t)cfg.maxTrace + 63) & ~63ull; }

void launchLongPass(hipStream_t stream, const DGraph& g, const CorrectnessTables* ct, const uint8_t* iupac, const ExtendConfig& cfg, const LongJob* jobs, uint32_t nReads,
	const LongSeed* seeds, const char* bases, uint64_t rcBase, uint32_t minClusterSize, uint32_t extraHeuristic, uint8_t* scratch, uint64_t slabBytes,
	LongCell* cellPool, unsigned long long* cellCursor, uint64_t cellCapacity, LongAln* alns, LongReadResult* results, unsigned long long* counters)
{
	if (nReads == 0) return;
	uint32_t blocks = (nReads + 63) / 64;
	if (cfg.clipOn())
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_long_pass<true, true>), dim3(blocks), dim3(64), 0, stream, g, ct, iupac, cfg, jobs, nReads, seeds, bases, rcBase, minClusterSize, extraHeuristic, scratch, slabBytes,
			cellPool, cellCursor, cellCapacity, alns, results, counters);
	else if (cfg.bandControls())
		hipLaunchKernelGGL(k_long_pass<true>, dim3(blocks), dim3(64), 0, stream, g, ct, iupac, cfg, jobs, nReads, seeds, bases, rcBase, minClusterSize, extraHeuristic, scratch, slabBytes,
			cellPool, cellCursor, cellCapacity, alns, results, counters);
	else
		hipLaunchKernelGGL(k_long_pass<false>, dim3(blocks), dim3(64), 0, stream, g, ct, iupac, cfg, jobs, nReads, seeds, bases, rcBase, minClusterSize, extraHeuristic, scratch, slabBytes,
			cellPool, cellCursor, cellCapacity, alns, results, counters);
}

void launchLongInit(hipStream_t stream, const LongJob* jobs, uint32_t nReads, LongState* state)
{
	if (nReads) hipLaunchKernelGGL(k_long_init, dim3((nReads + 255) / 256), dim3(256), 0, stream, jobs, nReads, state);
}
void launchLongSelect(hipStream_t stream, const DGraph& g, const LongJob* jobs, uint32_t nReads, const LongSeed* seeds, uint64_t rcBase, uint32_t minClusterSize, uint32_t extraHeuristic, uint32_t maxCandidates,
	LongState* state, const LongAln* alns, const LongCell* cellPool, LongWork* work, uint32_t* workLen, uint32_t* candSeed, unsigned long long* workCount, uint64_t workCapacity)
{
	if (maxCandidates < 1) maxCandidates = 1;
	if (maxCandidates > LONG_MAX_CANDIDATES) maxCandidates = LONG_MAX_CANDIDATES;
	if (nReads) hipLaunchKernelGGL(k_long_select, dim3(nReads), dim3(64), 0, stream, g, jobs, nReads, seeds, rcBase, minClusterSize, extraHeuristic, maxCandidates, state, alns, cellPool, work, workLen, candSeed, workCount, workCapacity);
}
void launchLongMerge(hipStream_t stream, const DGraph& g, const LongJob* jobs, uint32_t nReads, const LongSeed* seeds, const uint32_t* candSeed, const LongWorkResult* results,
	const unsigned long long* tracePool, LongState* state, LongAln* alns, LongCell* cellPool, unsigned long long* cellCursor, uint64_t cellCapacity, uint32_t extraHeuristic)
{
	if (nReads) hipLaunchKernelGGL(k_long_merge, dim3(nReads), dim3(64), 0, stream, g, jobs, nReads, seeds, candSeed, results, tracePool, state, alns, cellPool, cellCursor, cellCapacity, extraHeuristic);
}
void launchLongOrder(hipStream_t stream, const uint32_t* workLen, const unsigned long long* workCount, uint32_t* order, uint32_t maxLen, uint32_t mode)
{
	uint32_t shift = 0;
	while ((maxLen >> shift) > 1023) shift++;
	hipLaunchKernelGGL(k_long_order, dim3(1), dim3(GC_ORDER_THREADS), 0, stream, workLen, workCount, order, shift, mode);
}
void launchPublish(hipStream_t stream, const unsigned long long* src, unsigned long long* dst, uint32_t nWords)
{
	hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, stream, src, dst, nWords);
}
void launchZeroWords(hipStream_t stream, unsigned long long* dst, uint32_t nWords)
{
	hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, stream, dst, nWords);
}
void launchLongFinish(hipStream_t stream, uint32_t nReads, const LongState* state, LongReadResult* results)
{
	if (nReads) hipLaunchKernelGGL(k_long_finish, dim3((nReads + 255) / 256), dim3(256), 0, stream, nReads, state, results);
}

} // namespace gcdev
