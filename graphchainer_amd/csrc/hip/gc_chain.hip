// Co-linear chaining (K4): one wave per read, the working set in LDS (two size classes) or in the block's HBM scratch.
#include "gc_kernels.hpp"

namespace gcdev {

// =====================================================================================================
// K4 - co-linear chaining. reference: AlignmentGraph::colinearChaining / colinearChainingByComponent,
// src/AlignmentGraph.cpp:1712-1863. One wave per read.
//
// The reference sweeps anchor endpoints in topological order and keeps, per path k of the minimum path cover,
// two treaps keyed by read coordinate. What that sweep computes for anchor j is
//     C[j] = max( (len_j, -1),
//                 max_i (len_j + C[i].first, i)         over i with  y_i <  x_j      and  end(i) => start(j)
//                 max_i (y_j - y_i + C[i].first, i)     over i with  x_j <= y_i < y_j and  end(i) => start(j) )
// with lexicographic pair max (ties to the larger anchor index, :1812,1849) and  u => v  meaning "u strictly
// reaches v" (looked up through backwards[v], :1766,1834-1845) or "u == v and i sorts before j by (y,x)"
// (the node-local pass, :1785-1822). Both read conditions imply x_i < x_j, i.e. i belongs to an earlier
// fragment, and C[i] is final before any j of a later fragment reads it. So the same maxima can be taken in
// FRAGMENT order with a direct reachability test per pair, which needs no sort and no tables and is parallel
// over i: lanes scan the earlier anchors, a wave max-reduction yields C[j]. Anchor slots are already in
// fragment order. u strictly reaches v  <=>  some path k through u has pos_k(u) <= pos_k(last node of path k
// that strictly reaches v) - exactly the (node, k) pairs of backwards[v] (computeMPCIndex, :1373-1384).
// Cost O(n^2 K / 64) per read; n is a few hundred anchors.
// =====================================================================================================

#define CHAIN_NEEDS_SCRATCH 9u   // chainStatus between the two launches

__device__ __forceinline__ unsigned long long packScore(long long score, long long anchor)
{
	return ((unsigned long long)(score + (1ll << 30)) << 32) | (unsigned long long)(uint32_t)(anchor + 1);
}
__device__ __forceinline__ long long unpackScore(unsigned long long v) { return (long long)(v >> 32) - (1ll << 30); }
__device__ __forceinline__ long long unpackAnchor(unsigned long long v) { return (long long)(uint32_t)v - 1; }

// end(i) == u, start(j) == v, same weakly connected component already checked
__device__ __forceinline__ bool reachesStrictly(const DGraph& g, uint32_t u, uint32_t v)
{
	uint32_t pu = g.pathsOff[u], puEnd = g.pathsOff[u + 1];
	uint32_t bv = g.backOff[v], bvEnd = g.backOff[v + 1];
	while (pu < puEnd && bv < bvEnd) {   // both lists are ascending in path id
		uint32_t ku = g.paths[pu], kv = g.backPath[bv];
		if (ku == kv) {
			if (g.pathsPos[pu] <= g.backPos[bv]) return true;
			pu++; bv++;
		} else if (ku < kv) pu++;
		else bv++;
	}
	return false;
}

#define CHAIN_LDS_ANCHORS 1536
#define CHAIN_LDS_ENTRIES 2304
#define CHAIN_LDS_WIDTH 512

// Same maxima, without a reachability test per pair (r2). "end(i) strictly reaches start(j)" means: some path k of the cover runs
// through end(i) at a position <= the position of the last node of k that reaches start(j) - the (k, position) pairs of
// backwards[start(j)] (computeMPCIndex, :1373-1384). So every anchor i leaves one ENTRY (k, position of end(i) on k) per path
// through its end node, kept in LDS in anchor (= fragment) order, and anchor j is answered by one scan of the entries of earlier
// fragments against a small table thr[k] = position from backwards[start(j)] (-1 elsewhere): the reference's per-path treaps keyed
// by read coordinate, with the sweep order turned from topological to fragment order so that "earlier in the read" is a prefix.
// No global loads inside the DP loop (the pair-wise version fetched ~20x its input: two sorted lists merged per pair): entries and
// threshold lists of all anchors are laid out in LDS by the set-up pass, lanes in parallel.
struct ChainEntry { uint32_t pos; uint16_t k, anchor; };   // an anchor's end node on path k at position pos

struct ChainArrays {   // one read's working set: LDS (template LDS) or this block's HBM scratch
	uint32_t* aStart; unsigned long long* C;
	uint16_t* aFrag; uint16_t* aComp; uint16_t* entBegin; uint32_t* backBegin;
	ChainEntry* ent; uint2* back; int32_t* thr;   // back: the anchors' threshold lists (path, position), always in this block's HBM scratch (a wide cover makes them long)
	ChainEntry* entByComp; uint16_t* aBucket; uint16_t* entByCompBegin;   // scratch launch only (r4): the entries grouped by weakly connected component, see CHAIN_BUCKETS
	uint16_t* anchorByBucket;                                              // ... and (r5) the anchors grouped the same way, in anchor order inside a bucket
};
// r4, the scratch launch (reads with more anchors than the LDS classes hold - every 50 kb read): an anchor is only ever chained to anchors of its own weakly connected component, but the scan
// above visits the entries of ALL earlier anchors and drops the others one by one. On a 1 Gbp graph a 15-mer has a chance hit somewhere in the genome as often as not: a 50 kb read brings ~10 000
// anchors, most of them strays spread over the other chromosomes' components, and the scan was 3.1 s per 2 000 reads (`gpurun_out/r4_cfg5z`). The entries are therefore regrouped by component -
// component -> bucket through a 512-slot table, a counting sort that keeps the anchor order inside a bucket - and anchor j scans the part of its own bucket that earlier fragments filled.
// A read that touches more than 256 components keeps the plain scan.
#define CHAIN_BUCKETS 512u

// LDS == 0: the working set in this block's HBM scratch; 1: in LDS, the large class (53 KB: three blocks per CU); 2 (r4): in LDS, half the size (26.5 KB, six blocks per CU) - what a
// 10 kb read needs (~300 anchors, ~600 entries, cover width of a few) and the class launchChain picks when the batch's largest read fits it; a read that outgrows its class goes to the scratch launch
template <int LDS>
__global__ void __launch_bounds__(64) k_chain(DGraph g, const ReadChainJob* __restrict__ jobs, uint32_t nReads, const AnchorRec* __restrict__ anchors,
	const Fragment* __restrict__ frags, const uint32_t* __restrict__ fragStatus, int32_t splitLen, int32_t splitGap, ChainCaps caps, uint8_t* __restrict__ scratch, uint64_t scratchStride,
	uint32_t* __restrict__ chainOut, uint32_t* __restrict__ chainLen, unsigned long long* __restrict__ chainScore, uint32_t* __restrict__ chainStatus, uint32_t forceScratch)
{
	GC_RAISE_PRIO();
	constexpr uint32_t LDS_ANCHORS = LDS == 2 ? CHAIN_LDS_ANCHORS / 2 : CHAIN_LDS_ANCHORS, LDS_ENTRIES = LDS == 2 ? CHAIN_LDS_ENTRIES / 2 : CHAIN_LDS_ENTRIES, LDS_WIDTH = LDS == 2 ? CHAIN_LDS_WIDTH / 2 : CHAIN_LDS_WIDTH;
	__shared__ uint32_t sStart[LDS ? LDS_ANCHORS : 1];
	__shared__ unsigned long long sC[LDS ? LDS_ANCHORS : 1];
	__shared__ uint16_t sFrag[LDS ? LDS_ANCHORS : 1], sComp[LDS ? LDS_ANCHORS : 1], sEntBegin[LDS ? LDS_ANCHORS + 1 : 1];
	__shared__ uint32_t sBackBegin[LDS ? LDS_ANCHORS + 1 : 1];
	__shared__ ChainEntry sEnt[LDS ? LDS_ENTRIES : 1];
	__shared__ int32_t sThr[LDS ? LDS_WIDTH : 1];
	__shared__ uint32_t bKey[LDS ? 1 : CHAIN_BUCKETS], bStart[LDS ? 1 : CHAIN_BUCKETS + 1], bFilled[LDS ? 1 : CHAIN_BUCKETS], bUsed;   // bucket -> component, first entry, entries of earlier fragments
	__shared__ uint32_t bAnchors[LDS ? 1 : CHAIN_BUCKETS], bAnchorStart[LDS ? 1 : CHAIN_BUCKETS + 1], bAnchorsPlaced[LDS ? 1 : CHAIN_BUCKETS];   // (r5) anchors per bucket, and where the bucket's anchors begin in anchorByBucket
	constexpr uint32_t SCRATCH_THR = 2048;
	__shared__ int32_t sThrScratch[LDS ? 1 : SCRATCH_THR];   // (r5) the scratch launch's threshold table stays in LDS whenever the graph's widest path cover fits: it is scattered into, read per scanned entry and cleared for every anchor
	const int lane = threadIdx.x;
	// (16-bit indices: at most 65535 anchors, entries and threshold-list items per read, cover width and components below 65536; beyond that the read is flagged)
	const uint32_t capA = LDS ? LDS_ANCHORS : (caps.capAnchors < 65535u ? caps.capAnchors : 65535u);
	const uint32_t capE = LDS ? LDS_ENTRIES : (caps.capEndpoints < 65535u ? caps.capEndpoints : 65535u);
	const uint32_t capB = caps.capBack;
	const uint32_t capW = LDS ? LDS_WIDTH : (caps.capTable < 65535u ? caps.capTable : 65535u);
	ChainArrays A;
	uint8_t* base = scratch + (uint64_t)blockIdx.x * scratchStride;
	A.back = (uint2*)base; base += 8ull * capB;
	if (LDS) { A.aStart = sStart; A.C = sC; A.aFrag = sFrag; A.aComp = sComp; A.entBegin = sEntBegin; A.backBegin = sBackBegin; A.ent = sEnt; A.thr = sThr; }
	else {
		A.C = (unsigned long long*)base; base += 8ull * capA;
		A.ent = (ChainEntry*)base; base += 8ull * capE;
		A.aStart = (uint32_t*)base; base += 4ull * capA;
		A.backBegin = (uint32_t*)base; base += 4ull * (capA + 1);
		A.thr = (int32_t*)base; base += 4ull * capW;
		if (capW <= SCRATCH_THR) A.thr = sThrScratch;
		A.aFrag = (uint16_t*)base; base += 2ull * capA;
		A.aComp = (uint16_t*)base; base += 2ull * capA;
		A.entBegin = (uint16_t*)base; base += 2ull * (capA + 1);
		A.aBucket = (uint16_t*)base; base += 2ull * (capA + 1);
		A.entByCompBegin = (uint16_t*)base; base += 2ull * (capA + 1);
		A.anchorByBucket = (uint16_t*)base; base += 2ull * (capA + 1);
		base = (uint8_t*)(((uintptr_t)base + 7) & ~(uintptr_t)7);
		A.entByComp = (ChainEntry*)base;
	}
	for (uint32_t w = lane; w < capW; w += 64) A.thr[w] = -1;
	__syncthreads();
	for (uint32_t r = blockIdx.x; r < nReads; r += gridDim.x) {
		ReadChainJob job = jobs[r];
		if (!LDS && !(forceScratch & 4u) && chainStatus[r] != CHAIN_NEEDS_SCRATCH) continue;   // second launch: only the reads the LDS launch passed on (bit 2: there was no LDS launch - every read)
		// (r5) a read with more than twice the class's anchors in SLOTS is sent on without a look at its anchors: routing only - the scratch launch takes any read
		if (LDS && job.nSlots > 2 * LDS_ANCHORS) { if (lane == 0) { chainStatus[r] = CHAIN_NEEDS_SCRATCH; chainLen[r] = 0; chainScore[r] = 0; } continue; }
		// the reference never resets its `cont` flag after a fragment whose extension threw, so fragments after the
		// first failed one contribute no anchors (src/Aligner.cpp:695-703): slots from that fragment on are cut off
		uint32_t cut = job.nSlots;
		for (uint32_t f = lane; f < job.nFrags; f += 64)
			if (fragStatus[job.fragBegin + f] == 1) { uint32_t c = frags[job.fragBegin + f].seedBegin - job.slotBegin; cut = c < cut ? c : cut; }
		for (int d = 32; d > 0; d >>= 1) { uint32_t o = __shfl_xor(cut, d); cut = o < cut ? o : cut; }
		// Compact the read's valid anchors in slot order (== the order the reference pushes them, src/Aligner.cpp:706-721). Every anchor gets
		// its entries (one per path through its END node) and its threshold list: for its START node v, per path k the last position on k
		// that may precede it - backwards[v] (strict reachability, :1373-1384) plus (k, position of v) for the paths through v itself,
		// which adds "same node" (:1785-1822: an anchor of an earlier fragment ending in v sorts before j by (y, x)).
		uint32_t nA = 0, nE = 0, nB = 0;
		bool fits = !(LDS && forceScratch);   // test hook: every read through the scratch launch
		for (uint32_t s0 = 0; s0 < cut && fits; s0 += 64) {
			uint32_t s = s0 + lane;
			bool valid = false;
			AnchorRec rec;
			uint32_t pBegin = 0, pCount = 0, bBegin = 0, bCount = 0, vBegin = 0, vCount = 0, comp = 0;
			if (s < cut) { rec = anchors[job.slotBegin + s]; valid = rec.valid != 0; }
			if (valid) {
				pBegin = g.pathsOff[rec.lastNode]; pCount = g.pathsOff[rec.lastNode + 1] - pBegin;
				bBegin = g.backOff[rec.firstNode]; bCount = g.backOff[rec.firstNode + 1] - bBegin;
				vBegin = g.pathsOff[rec.firstNode]; vCount = g.pathsOff[rec.firstNode + 1] - vBegin;
				comp = g.componentMap[rec.lastNode];
			}
			unsigned long long ballot = __ballot(valid);
			uint32_t inclE = pCount, inclB = bCount + vCount;
			for (int d = 1; d < 64; d <<= 1) {
				uint32_t oe = __shfl_up(inclE, d), ob = __shfl_up(inclB, d);
				if (lane >= d) { inclE += oe; inclB += ob; }
			}
			const uint32_t chunkE = __shfl(inclE, 63), chunkB = __shfl(inclB, 63), chunkA = (uint32_t)__popcll(ballot);
			const bool wide = valid && (comp > 65535u || g.mpcWidth[comp] > capW || rec.x / (uint32_t)splitGap > 65535u);
			if (nA + chunkA > capA || nE + chunkE > capE || nB + chunkB > capB || __any(wide)) { fits = false; break; }
			if (valid) {
				const uint32_t a = nA + (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
				const uint32_t e0 = nE + inclE - pCount, t0 = nB + inclB - (bCount + vCount);
				A.aStart[a] = rec.firstNode;
				A.aFrag[a] = (uint16_t)(rec.x / (uint32_t)splitGap);   // fragment starts are multiples of the step: x and the index order alike
				A.aComp[a] = (uint16_t)comp;
				A.C[a] = packScore((long long)rec.y - (long long)rec.x + 1, -1);   // :1769
				A.entBegin[a] = (uint16_t)e0;
				A.backBegin[a] = t0;
				for (uint32_t i = 0; i < pCount; i++) A.ent[e0 + i] = ChainEntry { g.pathsPos[pBegin + i], (uint16_t)g.paths[pBegin + i], (uint16_t)a };
				for (uint32_t i = 0; i < bCount; i++) A.back[t0 + i] = make_uint2(g.backPath[bBegin + i], g.backPos[bBegin + i]);
				for (uint32_t i = 0; i < vCount; i++) A.back[t0 + bCount + i] = make_uint2(g.paths[vBegin + i], g.pathsPos[vBegin + i]);
			}
			nA += chunkA; nE += chunkE; nB += chunkB;
		}
		if (!fits) {
			if (lane == 0) { chainStatus[r] = LDS ? CHAIN_NEEDS_SCRATCH : 1u; chainLen[r] = 0; chainScore[r] = 0; }
			__syncthreads();
			continue;
		}
		if (lane == 0) { A.entBegin[nA] = (uint16_t)nE; A.backBegin[nA] = nB; }
		__syncthreads();
		bool bucketed = false;
		if (LDS == 0) {
			for (uint32_t b = lane; b < CHAIN_BUCKETS; b += 64) { bKey[b] = 0xffffffffu; bStart[b] = 0; bFilled[b] = 0; bAnchors[b] = 0; bAnchorsPlaced[b] = 0; }
			if (lane == 0) { bUsed = 0; bStart[CHAIN_BUCKETS] = 0; }
			__syncthreads();
			// component -> bucket (the slot its id hashes to), entries per bucket
			for (uint32_t a = lane; a < nA; a += 64) {
				const uint32_t comp = A.aComp[a];
				uint32_t slot = (comp * 2654435761u >> 16) & (CHAIN_BUCKETS - 1);
				for (uint32_t probes = 0; probes < CHAIN_BUCKETS; probes++, slot = (slot + 1) & (CHAIN_BUCKETS - 1)) {
					const uint32_t seen = atomicCAS(&bKey[slot], 0xffffffffu, comp);
					if (seen == 0xffffffffu) atomicAdd(&bUsed, 1u);
					if (seen == 0xffffffffu || seen == comp) break;
				}
				A.aBucket[a] = (uint16_t)slot;
				atomicAdd(&bStart[slot], (uint32_t)A.entBegin[a + 1] - (uint32_t)A.entBegin[a]);
				atomicAdd(&bAnchors[slot], 1u);
			}
			__syncthreads();
			bucketed = bUsed <= CHAIN_BUCKETS / 2 && !(forceScratch & 2u);   // (beyond that the probing may have wrapped: plain scan; bit 1 of forceScratch: test hook, plain scan)
			if (bucketed) {
				// exclusive scan of the counts (one wave, eight buckets per lane), then every anchor's place in its bucket in anchor order - lane 0, one pass
				uint32_t mine[CHAIN_BUCKETS / 64], sum = 0, mineA[CHAIN_BUCKETS / 64], sumA = 0;
				for (uint32_t k = 0; k < CHAIN_BUCKETS / 64; k++) { mine[k] = bStart[lane * (CHAIN_BUCKETS / 64) + k]; sum += mine[k]; mineA[k] = bAnchors[lane * (CHAIN_BUCKETS / 64) + k]; sumA += mineA[k]; }
				uint32_t incl = sum, inclA = sumA;
				for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d), oa = __shfl_up(inclA, d); if (lane >= d) { incl += o; inclA += oa; } }
				uint32_t at = incl - sum, atA = inclA - sumA;
				__syncthreads();
				for (uint32_t k = 0; k < CHAIN_BUCKETS / 64; k++) { bStart[lane * (CHAIN_BUCKETS / 64) + k] = at; at += mine[k]; bAnchorStart[lane * (CHAIN_BUCKETS / 64) + k] = atA; atA += mineA[k]; }
				__syncthreads();
				// every anchor's place in its bucket, in anchor order (r5: 64 anchors at a time - a lane adds up the entries of the chunk's earlier anchors that share its bucket from
				// the other lanes' registers, the buckets' fill counts advance by LDS atomics between chunks; r4 walked the read's ~10 000 anchors on lane 0 through its HBM scratch)
				for (uint32_t a0 = 0; a0 < nA; a0 += 64) {
					const uint32_t a = a0 + lane;
					const bool have = a < nA;
					const uint32_t slot = have ? (uint32_t)A.aBucket[a] : 0xffffffffu;
					const uint32_t cnt = have ? (uint32_t)A.entBegin[a + 1] - (uint32_t)A.entBegin[a] : 0u;
					uint32_t before = 0, anchorsBefore = 0;
					for (int l = 0; l < 63; l++) { const uint32_t s = __shfl(slot, l), c = __shfl(cnt, l); if (l < lane && s == slot) { before += c; anchorsBefore++; } }
					if (have) {
						A.entByCompBegin[a] = (uint16_t)(bStart[slot] + bFilled[slot] + before);
						A.anchorByBucket[bAnchorStart[slot] + bAnchorsPlaced[slot] + anchorsBefore] = (uint16_t)a;
					}
					__syncthreads();
					if (have) { if (cnt) atomicAdd(&bFilled[slot], cnt); atomicAdd(&bAnchorsPlaced[slot], 1u); }
					__syncthreads();
				}
				for (uint32_t b = lane; b < CHAIN_BUCKETS; b += 64) bFilled[b] = 0;
				__syncthreads();
				for (uint32_t a = lane; a < nA; a += 64)
					for (uint32_t e = A.entBegin[a], to = A.entByCompBegin[a]; e < A.entBegin[a + 1]; e++, to++) A.entByComp[to] = A.ent[e];
				__syncthreads();
			}
		}
		// anchors are ordered by fragment; g0 = first anchor of j's fragment, the entries of anchors < g0 are a prefix. The threshold lists
		// of consecutive anchors are consecutive in `back`: a 64-item window of them is kept in registers (item w0 + lane), refilled with one
		// coalesced load when an anchor's list runs past it - the only global access of the DP loop, a few times per hundred anchors on a narrow cover.
		uint32_t w0 = 0;
		uint2 win = (uint32_t)lane < nB ? A.back[lane] : make_uint2(0, 0);
		// one anchor's step: thr[k] = the last position on path k that may precede start(j) (its threshold list scattered into the table), the scan of the entries
		// [scanBegin, scanEnd) - earlier fragments' anchors - the wave maximum into C[j], the table cleared again. sameComponent: the entries are j's component's already
		auto relax = [&](uint32_t j, uint32_t fj, const ChainEntry* entries, uint32_t scanBegin, uint32_t scanEnd, bool sameComponent) {
			const uint32_t b0 = A.backBegin[j], b1 = A.backBegin[j + 1];
			if ((b0 >= w0 && b1 <= w0 + 64) || (b1 - b0 <= 64 && (w0 = b0, win = b0 + lane < nB ? A.back[b0 + lane] : make_uint2(0, 0), true))) {
				const uint32_t t = w0 + lane;
				if (t >= b0 && t < b1) atomicMax(&A.thr[win.x], (int32_t)win.y);
			} else {
				for (uint32_t t = b0 + lane; t < b1; t += 64) { const uint2 it = A.back[t]; atomicMax(&A.thr[it.x], (int32_t)it.y); }   // a list longer than the window (wide cover)
			}
			__syncthreads();
			const uint32_t compV = A.aComp[j];
			const long long xj = (long long)fj * splitGap, yj = xj + splitLen - 1;
			unsigned long long best = 0;
			for (uint32_t e = scanBegin + lane; e < scanEnd; e += 64) {
				const ChainEntry en = entries[e];
				const uint32_t i = en.anchor;
				if ((!sameComponent && A.aComp[i] != compV) || (int32_t)en.pos > A.thr[en.k]) continue;   // (path ids are per component)
				const long long yi = (long long)A.aFrag[i] * splitGap + splitLen - 1;
				const long long ci = unpackScore(A.C[i]);
				unsigned long long cand;
				if (yi <= xj - 1) cand = packScore((long long)splitLen + ci, i);
				else cand = packScore(yj - yi + ci, i);   // x_j <= y_i <= y_j - 1
				best = cand > best ? cand : best;
			}
			for (int d = 32; d > 0; d >>= 1) {
				unsigned long long o = __shfl_xor(best, d);
				best = o > best ? o : best;
			}
			if (lane == 0 && best > A.C[j]) A.C[j] = best;
			__syncthreads();
			if (b1 <= w0 + 64 && b0 >= w0) {
				const uint32_t t = w0 + lane;
				if (t >= b0 && t < b1) A.thr[win.x] = -1;
			} else {
				for (uint32_t t = b0 + lane; t < b1; t += 64) A.thr[A.back[t].x] = -1;
			}
		};
		// The read's chain (:1713-1733, :1847-1862): per component the lexicographic maximum of (coverage, anchor index); over the components, visited in ascending id, the first
		// strictly greater coverage - i.e. the largest coverage, among equals the smallest component id, inside it the largest anchor index: a wave maximum over the anchors of
		// coverage << 32 | (65535 - component) << 16 | anchor (r5; r4 let lane 0 walk all anchors twice per component - a million loads from the scratch for a 50 kb read that
		// touches fifty components)
		unsigned long long top = 0;
		auto topOver = [&](uint32_t count, auto anchorAt) {
			unsigned long long mine = 0;
			for (uint32_t q = lane; q < count; q += 64) {
				const uint32_t a = anchorAt(q);
				const unsigned long long key = ((unsigned long long)unpackScore(A.C[a]) << 32) | ((unsigned long long)(65535u - (uint32_t)A.aComp[a]) << 16) | a;
				mine = key > mine ? key : mine;
			}
			for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(mine, d); mine = o > mine ? o : mine; }
			top = mine > top ? mine : top;
		};
		if (LDS == 0 && bucketed) {
			// r5: component by component, the one with the most anchors first - and only while a component can still win: an anchor adds at most splitLen to a chain's coverage, so a
			// bucket of c anchors cannot reach more than c x splitLen. On a genome-sized graph a 50 kb read brings ~10 000 anchors of which ~1 400 lie where it comes from; the strays
			// on the other chromosomes' components (a few hundred each) never come near that component's coverage and used to cost six sevenths of the kernel. What is skipped has no
			// part in the result: the chain and its coverage are the winner's, C of the other components is never output.
			while (true) {
				uint32_t pick = 0;   // anchors << 10 | (1023 - slot): the fullest bucket not yet done, the lowest slot among equals
				for (uint32_t k = 0; k < CHAIN_BUCKETS / 64; k++) { const uint32_t slot = lane * (CHAIN_BUCKETS / 64) + k, c = bAnchors[slot]; const uint32_t key = c ? (c << 10) | (1023u - slot) : 0u; pick = key > pick ? key : pick; }
				for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(pick, d); pick = o > pick ? o : pick; }
				const uint32_t count = pick >> 10, slot = 1023u - (pick & 1023u);
				if (count == 0) break;
				if ((unsigned long long)count * (unsigned long long)splitLen < (top >> 32)) break;   // (an equal bound could still tie, and the smaller component id wins a tie: only strictly less is safe)
				__syncthreads();
				if (lane == 0) bAnchors[slot] = 0;
				const uint16_t* list = A.anchorByBucket + bAnchorStart[slot];
				const uint32_t entFirst = bStart[slot];
				uint32_t filled = 0, groupFrom = 0, fragPrev = 0;
				for (uint32_t q = 0; q < count; q++) {
					const uint32_t j = list[q];
					const uint32_t fj = A.aFrag[j];
					if (q > 0 && fj != fragPrev) {   // the fragment that just ended joins the prefix: C of its anchors is final
						uint32_t add = 0;
						for (uint32_t x = groupFrom + lane; x < q; x += 64) { const uint32_t a = list[x]; add += (uint32_t)A.entBegin[a + 1] - (uint32_t)A.entBegin[a]; }
						for (int d = 32; d > 0; d >>= 1) add += __shfl_xor(add, d);
						filled += add;
						groupFrom = q;
						__syncthreads();
					}
					fragPrev = fj;
					if (filled == 0) continue;
					relax(j, fj, A.entByComp, entFirst, entFirst + filled, true);
				}
				__syncthreads();
				topOver(count, [&](uint32_t q) { return (uint32_t)list[q]; });
			}
		} else {
			// anchors are ordered by fragment; g0 = first anchor of j's fragment, the entries of anchors < g0 are a prefix. The threshold lists
			// of consecutive anchors are consecutive in `back`: a 64-item window of them is kept in registers (item w0 + lane), refilled with one
			// coalesced load when an anchor's list runs past it - the only global access of the DP loop, a few times per hundred anchors on a narrow cover.
			uint32_t g0 = 0, entPrefix = 0;
			for (uint32_t j = 0; j < nA; j++) {
				const uint32_t fj = A.aFrag[j];
				if (j > 0 && fj != A.aFrag[j - 1]) { g0 = j; entPrefix = A.entBegin[j]; __syncthreads(); }   // C of the previous fragment's anchors is now final and visible
				if (g0 == 0) continue;
				relax(j, fj, A.ent, 0, entPrefix, false);
			}
			__syncthreads();
			topOver(nA, [&](uint32_t q) { return q; });
		}
		if (lane == 0) {
			uint32_t status = 0;
			const long long best = nA ? (long long)(top >> 32) : 0;
			uint32_t bestLen = 0;
			uint32_t* out = chainOut + job.chainBegin;
			if (nA) {
				uint32_t n = 0;
				for (long long i = (long long)(top & 0xffffu); i != -1; i = unpackAnchor(A.C[i])) {   // :1851-1862
					if (n >= job.nSlots) { status = 1; break; }
					out[n++] = (uint32_t)i;
				}
				for (uint32_t i = 0; i < n / 2; i++) { uint32_t t = out[i]; out[i] = out[n - 1 - i]; out[n - 1 - i] = t; }
				bestLen = n;
			}
			chainLen[r] = bestLen;
			chainScore[r] = (unsigned long long)best;
			chainStatus[r] = status;
		}
		__syncthreads();
	}
}

// =====================================================================================================
// launchers
// =====================================================================================================

uint64_t chainScratchBytes(const ChainCaps& caps)
{
	// the scratch launch's arrays for one read: anchors (capAnchors), entries (capEndpoints), threshold table (capTable)
	uint64_t b = 8ull * caps.capBack + 8ull * caps.capAnchors + 8ull * caps.capEndpoints + 4ull * caps.capAnchors + 4ull * (caps.capAnchors + 1) + 4ull * caps.capTable + 6ull * (caps.capAnchors + 1) + 256;
	b += 6ull * (caps.capAnchors + 1) + 8ull * caps.capEndpoints + 64;   // r4: bucket of every anchor, its entries' place by component, the entries in that order; r5: the anchors by bucket
	return (b + 63) & ~63ull;
}

uint32_t chainGridBlocks(uint32_t nReads) { return nReads < 2048 ? nReads : 2048; }   // three blocks fit a CU (LDS); every block owns a threshold-list region in HBM
uint32_t chainScratchBlocks(uint32_t nReads) { return nReads < 1024 ? nReads : 1024; }   // (r5: 1 024 - every block owns ~1.8 MB of scratch at config 5's read sizes, and the scratch launch is short since its DP runs per component)  r4:   // reads that do not fit the LDS tables: few on 10 kb reads (waves whose read is done leave at once), ALL of them on 50 kb reads (config 5: 256 blocks took 727 ms per 2 000 reads)

bool chainLdsLaunch(uint32_t fewestSlots, bool forceScratch) { return forceScratch || fewestSlots <= 2 * CHAIN_LDS_ANCHORS; }

void launchChain(hipStream_t stream, const DGraph& g, const ReadChainJob* jobs, uint32_t nReads, const AnchorRec* anchors, const Fragment* frags, const uint32_t* fragStatus,
	int32_t splitLen, int32_t splitGap, ChainCaps caps, uint8_t* scratch, uint32_t* chainOut, uint32_t* chainLen, unsigned long long* chainScore, uint32_t* chainStatus, bool plainScan, bool forceScratch, uint32_t fewestSlots)
{
	if (nReads == 0) return;
	// (r5) fewestSlots: the batch's smallest read in anchor slots. When even that one is beyond twice the large LDS class, the LDS launch would send every read on - 2 048 blocks of
	// 53 KB that waited up to 570 ms for LDS room among config 5's kernels to do nothing (`gpurun_out/r5_cfg5_c`): skipped, the scratch launch takes every read
	const bool ldsLaunch = chainLdsLaunch(fewestSlots, forceScratch);
	const uint32_t scratchFlags = (plainScan ? 2u : 0u) | (ldsLaunch ? 0u : 4u);
	// the half-size LDS class when the batch's largest read fits it (its entries are checked per read: a read with more goes to the scratch launch below)
	const bool small = caps.capAnchors <= CHAIN_LDS_ANCHORS / 2 && caps.capTable <= CHAIN_LDS_WIDTH / 2;
	if (!ldsLaunch) {}
	else if (small) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain<2>), dim3(chainGridBlocks(nReads)), dim3(64), 0, stream, g, jobs, nReads, anchors, frags, fragStatus, splitLen, splitGap, caps, scratch, chainScratchBytes(caps), chainOut, chainLen, chainScore, chainStatus, forceScratch ? 1u : 0u);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain<1>), dim3(chainGridBlocks(nReads)), dim3(64), 0, stream, g, jobs, nReads, anchors, frags, fragStatus, splitLen, splitGap, caps, scratch, chainScratchBytes(caps), chainOut, chainLen, chainScore, chainStatus, forceScratch ? 1u : 0u);
	// reads with more anchors / entries than the LDS tables hold, or on a cover wider than the LDS threshold table (waves whose read is done leave at once).
	// The batch's bounds tell when no read can need it (cfg2: 400 slots per read at most, cover width 2): 2 048 waves that look and leave cost 7 ms of queueing per batch.
	// (it is then a safety net of 64 waves for what the bounds do not show - a graph with more than 65 535 components, a read beyond 65 535 fragment positions; r5: eight waves
	// took 9-12 ms to look at 10 000 reads' status words, two dependent loads per read, in the fragment pipeline's critical path)
	const bool cannotBeNeeded = !forceScratch && caps.capAnchors <= CHAIN_LDS_ANCHORS / (small ? 2 : 1) && caps.capEndpoints <= CHAIN_LDS_ENTRIES / (small ? 2 : 1) && caps.capTable <= CHAIN_LDS_WIDTH / (small ? 2 : 1);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain<0>), dim3(cannotBeNeeded ? (nReads < 64 ? nReads : 64) : chainScratchBlocks(nReads)), dim3(64), 0, stream, g, jobs, nReads, anchors, frags, fragStatus, splitLen, splitGap, caps, scratch, chainScratchBytes(caps), chainOut, chainLen, chainScore, chainStatus, scratchFlags);
}

} // namespace gcdev
