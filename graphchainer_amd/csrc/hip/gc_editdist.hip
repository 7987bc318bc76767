// Path sequences and global (NW) edit distances on the GPU - SURVEY.md §8 row f1.
//
// The reference decides between the whole-read alignment and the chained alignment by two edit distances per read:
// edlibAlign(pathseq, read, EDLIB_MODE_NW) at src/Aligner.cpp:645 (path of the best whole-read alignment,
// traceToSequence :376-408,425-428) and at :845 (path of the stitched chain). edlib itself (edlib/src/edlib.cpp,
// Myers' bit-vector algorithm with Ukkonen's band) is a third-party component; only the VALUE it returns matters here,
// and the global edit distance of two strings is unique, so any exact algorithm is a drop-in for it.
//
// k_edit_distance: one wave per (path, read) pair. Rows = read bases, 64 per 64-bit word ("block"), columns = path
// letters. Lane l owns the units l, l+64, l+128, ... (unit = G consecutive blocks = 64G rows) and the wave sweeps the
// matrix as a skewed wavefront of column groups: at step t unit B works on the C columns of group t - B, so what unit B-1
// publishes after a group - its bottom row's score and the group's C horizontal deltas - is exactly what unit B needs one
// step later (two cross-lane shuffles per step). The step itself - corridor, windows, the C Myers columns, the final cell,
// the letter ring's refill rule - is gc_editdist_core.hpp, shared by the three kernels here and compiled for the host by
// tests/ed_host. Only the cells within Ukkonen's corridor are computed (the diagonals d = row - column with
// |d| + |(n - m) - d| <= k, about k of them, widened to whole groups); a unit enters with all-+1 vertical deltas below its
// upper neighbour and gets +1 as incoming horizontal delta when it is the top of the band. Band values are upper bounds
// and exact along every path of cost <= k, so a result <= k is the edit distance; otherwise k doubles and the pass
// repeats. k < 4000*G keeps a lane's consecutive units disjoint in time (edMaxBand; no limit when the read has at most
// 64 units, i.e. up to 4096*G rows); the host escalates G = 1, 2, 4, 8, 16.
#include "gc_kernels.hpp"
#include "gc_editdist_core.hpp"
#include <hip/hip_runtime.h>

namespace gcdev {

__device__ __forceinline__ char nodeLetter(const DGraph& g, uint32_t node, uint32_t pos)   // AlignmentGraph::NodeSequences, src/AlignmentGraph.cpp:751-796
{
	if (node < g.firstAmbiguous) {
		uint64_t w = g.nodeSeq[2 * (size_t)node + (pos >> 5)];
		const char acgt[4] = { 'A', 'C', 'G', 'T' };
		return acgt[(w >> ((pos & 31) * 2)) & 3];
	}
	const uint64_t* p = g.ambSeq + 4 * (size_t)(node - g.firstAmbiguous);
	uint32_t mask = (uint32_t)((p[0] >> pos) & 1) | (uint32_t)(((p[1] >> pos) & 1) << 1) | (uint32_t)(((p[2] >> pos) & 1) << 2) | (uint32_t)(((p[3] >> pos) & 1) << 3);
	const char iupac[16] = { 'N', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N' };
	return iupac[mask];
}

__device__ __forceinline__ uint32_t waveInclusiveScan(uint32_t v, uint32_t lane)
{
	for (int d = 1; d < 64; d <<= 1) {
		uint32_t o = __shfl_up(v, d);
		if ((int)lane >= d) v += o;
	}
	return v;
}

// traceToSequence (src/Aligner.cpp:376-408,425-428) of one alignment per read: the letters of the path between the first
// and the last trace cell. Cell j contributes the graph bases between the previous cell's position and its own, so the
// counts are independent, a wave scan places them, and every lane copies its own run.
__global__ void __launch_bounds__(64) k_long_pathseq(DGraph g, const PathSeqJob* __restrict__ jobs, uint32_t nJobs, const LongCell* __restrict__ cellPool,
	char* __restrict__ letters, uint32_t* __restrict__ outLen)
{
	GC_RAISE_ED_PRIO();
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= nJobs) return;
	const PathSeqJob job = jobs[r];
	if (job.count == 0) { if (lane == 0) outLen[r] = 0; return; }
	const LongCell* cells = cellPool + job.srcOff;
	char* out = letters + job.outOff;
	uint32_t total = 0;
	bool overflow = false;
	for (uint32_t base = 0; base < job.count; base += 64) {
		const uint32_t j = base + lane;
		uint32_t cnt = 0, node = 0, off = 0, prevNode = 0, prevOff = 0;
		if (j < job.count) {
			LongCell c = cells[j];
			node = g.lookup[g.lookupOff[c.node] + c.offset / 64];
			off = c.offset & 63u;
			if (j == 0) cnt = 1;
			else {
				LongCell p = cells[j - 1];
				prevNode = g.lookup[g.lookupOff[p.node] + p.offset / 64];
				prevOff = p.offset & 63u;
				if (node == prevNode) cnt = off > prevOff ? off - prevOff : 0;
				else cnt = ((uint32_t)g.nodeLength[prevNode] - (prevOff + 1)) + (off + 1);
			}
		}
		uint32_t incl = waveInclusiveScan(cnt, lane);
		uint32_t at = total + incl - cnt;
		if (at + cnt > job.outCap) overflow = true;
		else if (cnt) {
			uint32_t w = at;
			if (j == 0) out[w++] = nodeLetter(g, node, off);
			else if (node == prevNode) { for (uint32_t o = prevOff + 1; o <= off; o++) out[w++] = nodeLetter(g, node, o); }
			else {
				for (uint32_t o = prevOff + 1; o < g.nodeLength[prevNode]; o++) out[w++] = nodeLetter(g, prevNode, o);
				for (uint32_t o = 0; o <= off; o++) out[w++] = nodeLetter(g, node, o);
			}
		}
		total += __shfl(incl, 63);
	}
	if (__any(overflow)) total = 0xffffffffu;
	if (lane == 0) outLen[r] = total;
}

// pathToTrace (src/Aligner.cpp:409-424) of the stitched chain, as letters: first node from its start offset, last node
// (when it is not also the first) up to its last offset, whole nodes in between.
__global__ void __launch_bounds__(64) k_chain_pathseq(DGraph g, const PathSeqJob* __restrict__ jobs, uint32_t nJobs, const uint32_t* __restrict__ pathNodes,
	const uint32_t* __restrict__ altNodes, char* __restrict__ letters, uint32_t* __restrict__ outLen)
{
	GC_RAISE_ED_PRIO();
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= nJobs) return;
	const PathSeqJob job = jobs[r];
	if (job.count == 0) { if (lane == 0) outLen[r] = 0; return; }
	const uint32_t* nodes = (job.srcOff >> 63) ? altNodes + (job.srcOff & ~(1ull << 63)) : pathNodes + job.srcOff;   // bit 63: stitched on the host
	char* out = letters + job.outOff;
	uint32_t total = 0;
	bool overflow = false;
	for (uint32_t base = 0; base < job.count; base += 64) {
		const uint32_t i = base + lane;
		uint32_t S = 0, L = 0, node = 0;
		if (i < job.count) {
			node = nodes[i];
			L = g.nodeLength[node];
			if (i == 0) S = job.firstOffset;
			else if (i == job.count - 1) L = job.lastOffset + 1;
		}
		uint32_t cnt = L > S ? L - S : 0;
		uint32_t incl = waveInclusiveScan(cnt, lane);
		uint32_t at = total + incl - cnt;
		if (at + cnt > job.outCap) overflow = true;
		else for (uint32_t o = S; o < L; o++) out[at + (o - S)] = nodeLetter(g, node, o);
		total += __shfl(incl, 63);
	}
	if (__any(overflow)) total = 0xffffffffu;
	if (lane == 0) outLen[r] = total;
}

#define ED_RING 8192u

// the refill of a letter ring at the steps that are a multiple of PERIOD (gc_editdist_core.hpp): lane `first` of `stride` loads its share of the columns up to `end`
template <uint32_t RB, uint32_t C>
__device__ __forceinline__ void refillRing(uint8_t* ring, uint32_t ringMask, const EdBand& bd, const char* path, uint32_t tNext, uint32_t& loadedEnd, uint32_t first, uint32_t stride)
{
	const uint32_t end = edRingEnd<RB, C>(bd, tNext);
	if (end > loadedEnd) { edRingFill(ring, ringMask, path, bd.m, loadedEnd, end, first, stride); loadedEnd = end; }
}

// (waves per SIMD as before the column groups for units of 1, 2 and 4 words; units of 8 and 16 words - a few single-wave pairs of reads beyond 65 536 bases - keep their
// 96 and 192 registers of state out of scratch instead)
template <int G>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(G >= 8 ? 1 : G >= 4 ? 3 : G >= 2 ? 4 : 5))) k_edit_distance(const EdPair* __restrict__ pairs, uint32_t nPairs, const EdRead* __restrict__ reads, const char* __restrict__ bases,
	const uint64_t* __restrict__ eqMasks, const char* __restrict__ letters, const uint32_t* __restrict__ lettersLen, int64_t* __restrict__ outDistance)
{
	GC_RAISE_ED_PRIO();
	__shared__ __attribute__((aligned(8))) uint8_t ring[ED_RING];
	__shared__ int32_t resultSlot;
	const uint32_t lane = threadIdx.x;
	constexpr uint32_t C = edColsOfUnit(G), RB = 64u * G;   // columns per step, rows per unit
	constexpr uint32_t K_MAX = 4000u * G;             // the corridor is about k diagonals wide: a lane's consecutive units (64 units = 4096 G rows apart) stay disjoint in time
	constexpr uint32_t PERIOD = ED_RING / (2 * C);
	static_assert(K_MAX - 1 <= edMaxBand(RB, 64, C), "a lane's consecutive units must stay disjoint in time");
	for (uint32_t pi = blockIdx.x; pi < nPairs; pi += gridDim.x) {
		const EdPair pair = pairs[pi];
		const EdRead rd = reads[pair.read];
		const uint32_t n = rd.len;
		const uint32_t m = lettersLen ? lettersLen[pair.lenIndex] : pair.m;
		if (m == 0xffffffffu) { if (lane == 0) outDistance[pi] = -3; continue; }   // path letters overflowed their slot
		if (n == 0 || m == 0) { if (lane == 0) outDistance[pi] = (int64_t)(n + m); continue; }
		const EdSource src { eqMasks + rd.eqOff, rd.words, letters + pair.lettersOff, bases + rd.readOff, n, m };
		const uint32_t diff = n > m ? n - m : m - n;
		const uint32_t cap = n > m ? n : m;
		uint32_t k = pair.k > diff ? pair.k : diff;
		if (k < 1) k = 1;
		if (k > cap) k = cap;
		int64_t answer = -2;                         // -2: this G cannot hold the band, the host retries with a larger one
		while (true) {
			const EdBand bd = edBand<RB>(n, m, k);
			if (!edLanesHold(k, K_MAX, bd.nU, 64)) break;
			if (!edRingHolds<RB, C>(bd, ED_RING, PERIOD)) break;
			// ---- one banded pass
			EdUnit<G> u;
			uint32_t B = lane;                       // current unit of this lane
			bool fresh = true;                       // unit state not initialised yet
			EdPub pub { 0, 0 };
			uint32_t loadedEnd = 0;
			EdWindow w = edWindow<RB, C>(bd, B);      // per-unit step window, refreshed when the lane moves to its next unit
			if (lane == 0) resultSlot = -1;
			const uint32_t steps = (m - 1) / C + bd.nU;
			for (uint32_t t = 0; t < steps; t++) {
				if ((t & (PERIOD - 1)) == 0) {
					refillRing<RB, C>(ring, ED_RING - 1, bd, src.path, t + PERIOD, loadedEnd, lane, 64);
					__syncthreads();
				}
				EdPub nb;
				nb.score = __shfl(pub.score, (lane + 63) & 63);
				nb.bits = (uint32_t)__shfl((int)pub.bits, (lane + 63) & 63);
				if (B < bd.nU && t > w.tEnd) { do { B += 64; w = edWindow<RB, C>(bd, B); fresh = true; } while (B < bd.nU && t > w.tEnd); }
				if (t < w.tBegin) continue;
				int32_t d;
				if (edStep<C, G>(u, fresh, w, src, B, t, nb, ring, ED_RING - 1, pub, d)) resultSlot = d;
			}
			__syncthreads();
			const int32_t d = resultSlot;
			__syncthreads();
			if (d >= 0 && (uint32_t)d <= k) { answer = d; break; }
			if (k >= cap) { answer = d; break; }    // the band already covers the whole matrix
			const uint32_t failedK = k;
			k = k * 2 < cap ? k * 2 : cap;
			// no kernel is wider than the unit of 16 words: before it gives a pair up, it tries the widest band its lanes hold (a read of 65 700 bases 32 020 edits from its
			// path, first band 32 000: twice that is beyond the lanes, 63 999 is not)
			if (G == 16 && failedK < K_MAX - 1 && !edLanesHold(k, K_MAX, bd.nU, 64)) k = K_MAX - 1;
		}
		if (lane == 0) outDistance[pi] = answer;
	}
}

// Several pairs per wave (unit of one block): the corridor of a 10 kb pair is 16-23 units wide, so a wave with one pair keeps a third of its
// lanes busy and its time is set by the number of steps (column groups + units), not by the band. The wave is cut into teams of TEAM lanes - 32: two
// pairs, bands up to k = 1900; 21: three pairs (one lane idles), bands up to k = 1441, which a 10 kb read's whole-read pair and nearly all chain pairs
// fit - and every team sweeps its own pair: lane l of a team owns the units l, l + TEAM, ... (a lane's consecutive units are disjoint in
// time while k <= edMaxBand(64, TEAM, C)), the neighbour shuffle stays inside the team, each team has its own letter ring and result slot, and the teams
// step together (a team that is done, or has a shorter pair, idles). Same arithmetic as k_edit_distance<1>; a pair whose band would outgrow the
// team answers -2 and is rerun by the host with the wider kernels.
// (waves per SIMD as before the column groups, 5 and 4: the registers that costs are pair constants, spilled where a unit is entered and where a letter is no ACGT)
template <uint32_t TEAM, uint32_t RING>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TEAM >= 32 ? 4 : 5))) k_edit_distance_team(const EdPair* __restrict__ pairs, uint32_t nPairs, const EdRead* __restrict__ reads, const char* __restrict__ bases,
	const uint64_t* __restrict__ eqMasks, const char* __restrict__ letters, const uint32_t* __restrict__ lettersLen, int64_t* __restrict__ outDistance)
{
	GC_RAISE_ED_PRIO();
	constexpr uint32_t C = ED_COLS, RB = 64u, PAIRS = 64u / TEAM, KMAX = TEAM >= 32 ? ED_HALF_KMAX : ED_THIRD_KMAX, PERIOD = RING / (2 * C);
	static_assert(KMAX - 1 <= edMaxBand(RB, TEAM, C), "a lane's consecutive units must stay disjoint in time");
	__shared__ __attribute__((aligned(8))) uint8_t ringAll[(PAIRS + 1) * RING];   // (+ 1: the lanes beyond the last whole team address a ring of their own and never touch it)
	__shared__ int32_t resultSlot[PAIRS + 1];
	const uint32_t lane = threadIdx.x, half = lane / TEAM, l = lane - half * TEAM;
	uint8_t* ring = ringAll + half * RING;
	for (uint32_t base = blockIdx.x * PAIRS; base < nPairs; base += gridDim.x * PAIRS) {
		const uint32_t pi = base + half;
		const bool valid = half < PAIRS && pi < nPairs;
		EdPair pair {};
		EdRead rd {};
		uint32_t n = 0, m = 0;
		if (valid) {
			pair = pairs[pi];
			rd = reads[pair.read];
			n = rd.len;
			m = lettersLen ? lettersLen[pair.lenIndex] : pair.m;
		}
		int64_t answer = -2;
		bool more = valid;
		if (valid && m == 0xffffffffu) { answer = -3; more = false; }            // path letters overflowed their slot
		else if (valid && (n == 0 || m == 0)) { answer = (int64_t)(n + m); more = false; }
		const EdSource src { eqMasks + rd.eqOff, rd.words, letters + pair.lettersOff, bases + rd.readOff, n, m };
		const uint32_t diff = n > m ? n - m : m - n;
		const uint32_t cap = n > m ? n : m;
		uint32_t k = pair.k > diff ? pair.k : diff;
		if (k < 1) k = 1;
		if (k > cap) k = cap;
		while (__any(more)) {
			EdBand bd = edBand<RB>(n, m, k);
			if (more && !(edLanesHold(k, KMAX, bd.nU, TEAM) && edRingHolds<RB, C>(bd, RING, PERIOD))) more = false;   // -2: the wider kernels take it
			if (!more) bd.nU = 0;                                                 // (no unit, no window, no step)
			// ---- one banded pass of every half that still has one to do
			EdUnit<1> u;
			uint32_t B = l;
			bool fresh = true;
			EdPub pub { 0, 0 };
			uint32_t loadedEnd = 0;
			EdWindow w = edWindow<RB, C>(bd, B);
			if (l == 0 && half < PAIRS) resultSlot[half] = -1;
			const uint32_t steps = more ? (m - 1) / C + bd.nU : 0;
			uint32_t allSteps = steps;
			for (int d = 32; d >= 1; d >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)allSteps, d); allSteps = other > allSteps ? other : allSteps; }
			const int neighbour = (int)(half * TEAM + (l + TEAM - 1) % TEAM);
			for (uint32_t t = 0; t < allSteps; t++) {
				if ((t & (PERIOD - 1)) == 0) {
					if (more) refillRing<RB, C>(ring, RING - 1, bd, src.path, t + PERIOD, loadedEnd, l, TEAM);
					__syncthreads();
				}
				EdPub nb;
				nb.score = __shfl(pub.score, neighbour);
				nb.bits = (uint32_t)__shfl((int)pub.bits, neighbour);
				if (B < bd.nU && t > w.tEnd) { do { B += TEAM; w = edWindow<RB, C>(bd, B); fresh = true; } while (B < bd.nU && t > w.tEnd); }
				if (t < w.tBegin) continue;
				int32_t d;
				if (edStep<C, 1>(u, fresh, w, src, B, t, nb, ring, RING - 1, pub, d)) resultSlot[half] = d;
			}
			__syncthreads();
			const int32_t d = resultSlot[half];
			__syncthreads();
			if (more) {
				if (d >= 0 && (uint32_t)d <= k) { answer = d; more = false; }
				else if (k >= cap) { answer = d; more = false; }
				else k = k * 2 < cap ? k * 2 : cap;
			}
		}
		if (l == 0 && valid) outDistance[pi] = answer;
	}
}

// The whole matrix by one WORKGROUP (r4): thread B owns the 64 rows of block B for every column group, the threads sweep the matrix as one skewed wavefront (block B is on group t - B
// at step t) and hand the group's horizontal deltas of their bottom row to the next thread through LDS, one barrier per step. For the pairs whose band would cover most of the matrix anyway - a
// chain whose path spells a fraction of its read (distance >= the length difference), a whole-read alignment of a sliver of its read: the banded kernels give such a pair ONE wave
// with up to sixteen blocks per lane and step (config 5: a 50 000 x 1 000 pair held its stream for 385 ms; cfg2: ~800 pairs per batch in k_edit_distance<4>, 11.8 ms alone). Here a
// pair takes column groups + blocks steps of one block each, and every pair of the latter kind gets its own waves. No band, no retry: the result is exact.
#define ED_BLOCK_THREADS 1024u
#define ED_BLOCK_RING 16384u
__global__ void __launch_bounds__(ED_BLOCK_THREADS) k_edit_distance_block(const EdPair* __restrict__ pairs, uint32_t nPairs, const EdRead* __restrict__ reads, const char* __restrict__ bases,
	const uint64_t* __restrict__ eqMasks, const char* __restrict__ letters, const uint32_t* __restrict__ lettersLen, int64_t* __restrict__ outDistance)
{
	GC_RAISE_ED_PRIO();
	constexpr uint32_t C = ED_COLS, PERIOD = ED_BLOCK_RING / (2 * C);
	static_assert((PERIOD + ED_BLOCK_THREADS - 1) * C <= ED_BLOCK_RING, "the ring holds the group of the last block when it is refilled for the first");
	__shared__ __attribute__((aligned(8))) uint8_t ring[ED_BLOCK_RING];
	__shared__ uint32_t hand[2][ED_BLOCK_THREADS];   // the horizontal deltas leaving block B's bottom row in the group it has just computed, double-buffered by step parity
	__shared__ int32_t resultSlot;
	const uint32_t B = threadIdx.x;
	for (uint32_t pi = blockIdx.x; pi < nPairs; pi += gridDim.x) {
		const EdPair pair = pairs[pi];
		const EdRead rd = reads[pair.read];
		const uint32_t n = rd.len;
		const uint32_t m = lettersLen ? lettersLen[pair.lenIndex] : pair.m;
		if (m == 0xffffffffu) { if (B == 0) outDistance[pi] = -3; continue; }   // path letters overflowed their slot
		if (n == 0 || m == 0) { if (B == 0) outDistance[pi] = (int64_t)(n + m); continue; }
		const uint32_t nU = (n + 63u) / 64u;
		if (nU > blockDim.x) { if (B == 0) outDistance[pi] = -2; continue; }       // (the host sends only pairs that fit: -2 = the banded kernels take it)
		const EdSource src { eqMasks + rd.eqOff, rd.words, letters + pair.lettersOff, bases + rd.readOff, n, m };
		const EdBand bd = edBand<64>(n, m, n > m ? n : m);
		const EdWindow w = edWindowFull<C>(bd, B);
		const uint32_t mPad = (m + C - 1) / C * C;
		EdUnit<1> u;
		edEnter<1>(u, src, B < nU ? B : 0);
		u.score = (int32_t)(64u * (B + 1));                                        // every block starts on column 0: D[i][-1] = i + 1
		bool fresh = false;
		EdPub pub { 0, 0 };
		uint32_t loadedEnd = 0;
		const uint32_t steps = (m - 1) / C + nU;
		if (B == 0) resultSlot = -1;
		for (uint32_t t = 0; t < steps; t++) {
			if ((t & (PERIOD - 1)) == 0) {           // (the barrier that ended the step before keeps these writes behind its reads)
				const uint64_t want = (uint64_t)(t + PERIOD) * C;
				const uint32_t end = want < mPad ? (uint32_t)want : mPad;
				if (end > loadedEnd) { edRingFill(ring, ED_BLOCK_RING - 1, src.path, m, loadedEnd, end, B, blockDim.x); loadedEnd = end; }
				__syncthreads();
			}
			if (t >= w.tBegin && t <= w.tEnd) {
				EdPub nb { 0, B > 0 ? hand[(t + 1) & 1][B - 1] : 0u };   // (every block starts on group 0: the neighbour's score is never asked for)
				int32_t d;
				if (edStep<C, 1>(u, fresh, w, src, B, t, nb, ring, ED_BLOCK_RING - 1, pub, d)) resultSlot = d;
				hand[t & 1][B] = pub.bits;
			}
			__syncthreads();
		}
		if (B == 0) outDistance[pi] = (int64_t)resultSlot;
		__syncthreads();
	}
}

void launchEditDistanceBlock(hipStream_t stream, uint32_t threads, const EdPair* pairs, uint32_t nPairs, const EdRead* reads, const char* bases, const uint64_t* eqMasks,
	const char* letters, const uint32_t* lettersLen, int64_t* outDistance)
{
	if (!nPairs) return;
	threads = ((threads < 64u ? 64u : threads) + 63u) & ~63u;
	if (threads > ED_BLOCK_THREADS) threads = ED_BLOCK_THREADS;
	hipLaunchKernelGGL(k_edit_distance_block, dim3(nPairs < 65536u ? nPairs : 65536u), dim3(threads), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance);
}
uint32_t editDistanceBlockMaxRows() { return 64u * ED_BLOCK_THREADS; }

void launchLongPathSeq(hipStream_t stream, const DGraph& g, const PathSeqJob* jobs, uint32_t nJobs, const LongCell* cellPool, char* letters, uint32_t* outLen)
{
	if (nJobs) hipLaunchKernelGGL(k_long_pathseq, dim3(nJobs), dim3(64), 0, stream, g, jobs, nJobs, cellPool, letters, outLen);
}
void launchChainPathSeq(hipStream_t stream, const DGraph& g, const PathSeqJob* jobs, uint32_t nJobs, const uint32_t* pathNodes, const uint32_t* altNodes, char* letters, uint32_t* outLen)
{
	if (nJobs) hipLaunchKernelGGL(k_chain_pathseq, dim3(nJobs), dim3(64), 0, stream, g, jobs, nJobs, pathNodes, altNodes, letters, outLen);
}
uint32_t editDistanceMaxK(uint32_t unitBlocks) { return unitBlocks == 0 ? ED_HALF_KMAX : 4000u * unitBlocks; }   // unit 0: the two-pairs-per-wave kernel
uint32_t editDistanceTeamMaxK(uint32_t pairsPerWave) { return pairsPerWave == 3 ? ED_THIRD_KMAX : ED_HALF_KMAX; }
void launchEditDistanceTeam(hipStream_t stream, uint32_t pairsPerWave, const EdPair* pairs, uint32_t nPairs, const EdRead* reads, const char* bases, const uint64_t* eqMasks,
	const char* letters, const uint32_t* lettersLen, int64_t* outDistance)
{
	if (!nPairs) return;
	const uint32_t waves = (nPairs + pairsPerWave - 1) / pairsPerWave, blocks = waves < 65536 ? waves : 65536;
	if (pairsPerWave == 3) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_edit_distance_team<21, 2048>), dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_edit_distance_team<32, 4096>), dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance);
}
void launchEditDistance(hipStream_t stream, uint32_t unitBlocks, const EdPair* pairs, uint32_t nPairs, const EdRead* reads, const char* bases, const uint64_t* eqMasks,
	const char* letters, const uint32_t* lettersLen, int64_t* outDistance)
{
	if (!nPairs) return;
	uint32_t blocks = nPairs < 65536 ? nPairs : 65536;
	if (unitBlocks == 0) { launchEditDistanceTeam(stream, 2, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); return; }   // two pairs per wave (launchEditDistances sends the pairs with a small first band here)
	switch (unitBlocks) {
		case 1: hipLaunchKernelGGL(k_edit_distance<1>, dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); break;
		case 2: hipLaunchKernelGGL(k_edit_distance<2>, dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); break;
		case 4: hipLaunchKernelGGL(k_edit_distance<4>, dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); break;
		case 8: hipLaunchKernelGGL(k_edit_distance<8>, dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); break;
		default: hipLaunchKernelGGL(k_edit_distance<16>, dim3(blocks), dim3(64), 0, stream, pairs, nPairs, reads, bases, eqMasks, letters, lettersLen, outDistance); break;
	}
}

} // namespace gcdev
