// The chained alignment of --fast-mode (gc_params::fast_mode; src/Aligner.cpp:834-843,880-895): no edlib. The trace is the stitched piece itself,
// `longest` = pathToTrace(pos_path, firstNodeOffset, lastNodeOffset) (:409-424), one cell per path base; cell j sits at read position
// min(y, x + j) with x = A[ids[0]].x and y = A[ids.back()].y, and the alignment's score is the number of cells whose graph letter is not the
// read's letter at that position (chars compared as they are: IUPAC letters of ambiguous nodes count like any other).
//
// Two kernels, one wave per job, a job's work a function of its own record alone:
//   k_fast_chain_score   for every read with a stitched piece: the count, from the letters k_chain_pathseq has spelled for the NW distance
//                        of the default mode (the same cells in the same order, so nothing is walked twice)
//   k_fast_chain_trace   for the reads whose trace is wanted: node id, offset, read position and node switch of every cell in output
//                        coordinates (:880-887), into arrays laid out like gc_result::chain_trace_*
// Every store is a plain vector store; the only cross-lane traffic is the wave scan over the node lengths and the shuffles that hand a
// cell's node to the lane that writes it.
#include "gc_kernels.hpp"
#include <hip/hip_runtime.h>

namespace gcdev {

__global__ void __launch_bounds__(64) k_fast_chain_score(const FastChainJob* __restrict__ jobs, uint32_t nJobs, const char* __restrict__ letters, const uint32_t* __restrict__ lettersLen,
	const char* __restrict__ bases, int64_t* __restrict__ outScore)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= nJobs) return;
	const FastChainJob job = jobs[r];
	if (job.cells == 0) { if (lane == 0) outScore[r] = -1; return; }                       // no stitched piece: no chained alignment
	if (lettersLen[r] != job.cells) { if (lane == 0) outScore[r] = -3; return; }           // k_chain_pathseq did not spell what path_cells counts
	const char* path = letters + job.lettersOff;
	const char* read = bases + job.readOff;
	uint32_t differ = 0;
	for (uint32_t base = 0; base < job.cells; base += 64) {
		const uint32_t j = base + lane;
		bool d = false;
		if (j < job.cells) {
			const uint32_t want = job.x + j;                                                 // (x < y < read length < 2^32 - cells: no wrap)
			d = path[j] != read[want < job.y ? want : job.y];                                // seqPos = min(y, x + j), :838
		}
		differ += (uint32_t)__popcll(__ballot(d));
	}
	if (lane == 0) outScore[r] = (int64_t)differ;
}

__global__ void __launch_bounds__(64) k_fast_chain_trace(DGraph g, const FastChainJob* __restrict__ jobs, uint32_t nJobs, const uint32_t* __restrict__ pathNodes,
	const uint32_t* __restrict__ altNodes, int32_t* __restrict__ traceNode, uint32_t* __restrict__ traceOffset, uint32_t* __restrict__ traceSeqPos, uint8_t* __restrict__ traceSwitch,
	uint32_t* __restrict__ written)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= nJobs) return;
	const FastChainJob job = jobs[r];
	const uint32_t* nodes = (job.srcOff >> 63) ? altNodes + (job.srcOff & ~(1ull << 63)) : pathNodes + job.srcOff;   // bit 63: stitched on the host
	uint32_t total = 0;                                // cells of the nodes before this turn
	for (uint32_t nb = 0; nb < job.count; nb += 64) {
		// 64 path nodes per turn, as k_chain_pathseq cuts them (pathToTrace :412-416: a one-node piece runs to the node's end)
		const uint32_t i = nb + lane;
		uint32_t S = 0, L = 0, node = 0;
		if (i < job.count) {
			node = nodes[i];
			L = g.nodeLength[node];
			if (i == 0) S = job.firstOffset;
			else if (i == job.count - 1) L = job.lastOffset + 1;
		}
		const uint32_t cnt = L > S ? L - S : 0;
		uint32_t incl = cnt;
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t o = __shfl_up(incl, d);
			if ((int)lane >= d) incl += o;
		}
		const uint32_t turnCells = __shfl(incl, 63);
		const int32_t id = i < job.count ? g.nodeIDs[node] : 0;                              // :886-887 output coordinates
		const uint32_t first = i < job.count ? g.nodeOffset[node] + S : 0;                   // the node's first cell, as an offset in the original node
		// the turn's cells, 64 at a time, one per lane: the node a cell lies in is the first whose inclusive sum passes the cell's index
		for (uint32_t c0 = 0; c0 < turnCells; c0 += 64) {
			const uint32_t c = c0 + lane < turnCells ? c0 + lane : turnCells - 1;
			uint32_t owner = 0;
			for (uint32_t step = 32; step; step >>= 1) {
				const uint32_t v = __shfl(incl, (int)(owner + step - 1));
				if (v <= c) owner += step;
			}
			const uint32_t oIncl = __shfl(incl, (int)owner), oCnt = __shfl(cnt, (int)owner), oFirst = __shfl(first, (int)owner);
			const int32_t oId = __shfl(id, (int)owner);
			const uint32_t k = c - (oIncl - oCnt);                                           // the cell's place inside its node's run
			const uint32_t j = total + c;                                                    // ... and inside the piece
			if (c0 + lane < turnCells && j < job.cells) {                                    // (never beyond what the host reserved for the job)
				const uint64_t at = job.traceOff + j;
				const uint32_t want = job.x + j;
				traceNode[at] = oId;
				traceOffset[at] = oFirst + k;
				traceSeqPos[at] = want < job.y ? want : job.y;
				traceSwitch[at] = (k + 1 == oCnt && j + 1 < job.cells) ? 1 : 0;              // :880-883: the next cell lies in another split node
			}
		}
		total += turnCells;
	}
	if (lane == 0) written[r] = total;                 // == job.cells, or the host refuses the batch
}

void launchFastChainScore(hipStream_t stream, const FastChainJob* jobs, uint32_t nJobs, const char* letters, const uint32_t* lettersLen, const char* bases, int64_t* outScore)
{
	if (nJobs) hipLaunchKernelGGL(k_fast_chain_score, dim3(nJobs), dim3(64), 0, stream, jobs, nJobs, letters, lettersLen, bases, outScore);
}

void launchFastChainTrace(hipStream_t stream, const DGraph& g, const FastChainJob* jobs, uint32_t nJobs, const uint32_t* pathNodes, const uint32_t* altNodes,
	int32_t* traceNode, uint32_t* traceOffset, uint32_t* traceSeqPos, uint8_t* traceSwitch, uint32_t* written)
{
	if (nJobs) hipLaunchKernelGGL(k_fast_chain_trace, dim3(nJobs), dim3(64), 0, stream, g, jobs, nJobs, pathNodes, altNodes, traceNode, traceOffset, traceSeqPos, traceSwitch, written);
}

} // namespace gcdev
