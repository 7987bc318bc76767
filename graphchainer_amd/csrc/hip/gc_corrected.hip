// Corrected reads on the device (gc_params::device_output & 8): GraphAligner's --corrected-out / --corrected-clipped-out, whose mechanism the reference still carries
// (AddCorrected src/GraphAligner.h:220-231, getCorrected src/ReadCorrection.cpp:38-64, the writers src/Aligner.cpp:313-374). The piece of an alignment is the graph's
// letters along its trace with the insertions left out - a third reading of the cells the GAF / vg encoder walks (gc_output.hip), and like it done where the traces are:
// only the letters come down, about one byte per read base, instead of 16 bytes per trace cell.
//
// One wave per final alignment, 64 cells per step. A lane keeps its cell by corrKeeps (gc_corrected_core.hpp) from its own cell and the one before it - the neighbour
// lane's, or for lane 0 the last cell of the previous chunk, carried in a register. A ballot of the keep flags and a popcount of the bits below the lane place the letters.
// House form (gc_output.hip): <false> counts the letters of every job, k_corr_place scans the counts over the jobs, <true> writes. No atomics on the output, no scratch,
// no LDS in the walking kernel. The counting pass never touches the graph; the writing pass looks a letter up only for the cells it keeps.
// Its own kernels, not a branch of k_out_encode: that kernel's registers and time are the benchmark's, and bit 8 is off there.
// Compiler's resource summary (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_corr_walk<false> 15 VGPRs, <true> 26 VGPRs, k_corr_place 46 VGPRs and 8 KB of LDS;
// scratch 0 bytes per lane, 0 SGPR and 0 VGPR spills, occupancy 8 waves per SIMD for all three.
#include "gc_kernels.hpp"
#include "gc_corrected_core.hpp"
#include <hip/hip_runtime.h>

namespace gcdev {

namespace {

// the set of plain bases under (bigraph node, offset in the original node), as in gc_output.hip - but the raw column: an all-zero one stays 0, which corrLetter spells 'N'
__device__ __forceinline__ uint32_t corrGraphSet(const DGraph& g, int32_t nodeId, uint32_t offset)
{
	const uint32_t split = g.lookup[g.lookupOff[nodeId] + (offset >> 6)];
	const uint32_t pos = offset & 63u;
	if (split < g.firstAmbiguous) return 1u << ((g.nodeSeq[2 * (size_t)split + (pos >> 5)] >> ((pos & 31u) * 2)) & 3u);
	const uint64_t* p = g.ambSeq + 4 * (size_t)(split - g.firstAmbiguous);
	return (uint32_t)((p[0] >> pos) & 1) | (uint32_t)(((p[1] >> pos) & 1) << 1) | (uint32_t)(((p[2] >> pos) & 1) << 2) | (uint32_t)(((p[3] >> pos) & 1) << 3);
}

} // namespace

// lens[j]: letters of job j's piece (counting pass). The writing pass puts them at text + offsets[j] and sets lens[j] = ~0u if it did not land on that count.
template <bool WRITE>
__global__ void __launch_bounds__(64) k_corr_walk(DGraph g, const OutJob* __restrict__ jobs, uint32_t nJobs, const LongCell* __restrict__ cellPool, uint32_t* __restrict__ lens,
	const uint64_t* __restrict__ offsets, char* __restrict__ text)
{
	const uint32_t j = blockIdx.x, lane = threadIdx.x;
	if (j >= nJobs) return;
	const uint32_t n = jobs[j].cellLen;
	if (n == 0) { if (!WRITE && lane == 0) lens[j] = 0; return; }
	const LongCell* cells = cellPool + jobs[j].cellOff;
	char* out = WRITE ? text + offsets[j] : nullptr;
	int32_t carryNode = 0; uint32_t carryOffset = 0, carrySwitch = 0;   // the cell before this chunk's first
	uint32_t cur = 0;                                                   // letters so far
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t pos = base + lane;
		const bool valid = pos < n;
		const uint32_t nValid = n - base < 64 ? n - base : 64;
		const LongCell c = cells[valid ? pos : n - 1];
		int32_t pNode = __shfl_up(c.node, 1); uint32_t pOffset = __shfl_up(c.offset, 1), pSwitch = __shfl_up(c.nodeSwitch, 1);
		if (lane == 0) { pNode = carryNode; pOffset = carryOffset; pSwitch = carrySwitch; }
		const bool keep = valid && corrKeeps(pos == 0, pNode, pOffset, pSwitch, c.node, c.offset);
		const uint64_t keepMask = __ballot(keep);
		if (WRITE && keep) out[cur + corrRank(keepMask, lane)] = corrLetter(corrGraphSet(g, c.node, c.offset));
		cur += (uint32_t)__popcll(keepMask);
		carryNode = __shfl(c.node, (int)nValid - 1); carryOffset = __shfl(c.offset, (int)nValid - 1); carrySwitch = __shfl(c.nodeSwitch, (int)nValid - 1);
	}
	if (lane == 0) {
		if (!WRITE) lens[j] = cur;
		else if (cur != lens[j]) lens[j] = 0xffffffffu;   // the writing pass must land exactly where the counting pass said it would
	}
}

// exclusive scan of the counts over the jobs -> offsets[nJobs + 1] (the last entry and *total = the sum); one block
__global__ void __launch_bounds__(1024) k_corr_place(const uint32_t* __restrict__ lens, uint32_t nJobs, uint64_t* __restrict__ offsets, unsigned long long* __restrict__ total)
{
	__shared__ unsigned long long part[1024];
	const uint32_t t = threadIdx.x;
	const uint32_t per = (nJobs + 1023) / 1024;
	const uint32_t b = (uint64_t)t * per < nJobs ? t * per : nJobs, e = (uint64_t)b + per < nJobs ? b + per : nJobs;
	unsigned long long s = 0;
	for (uint32_t i = b; i < e; i++) s += lens[i];
	part[t] = s;
	__syncthreads();
	if (t == 0) {
		unsigned long long run = 0;
		for (uint32_t i = 0; i < 1024; i++) { const unsigned long long v = part[i]; part[i] = run; run += v; }
		offsets[nJobs] = run;
		*total = run;
	}
	__syncthreads();
	unsigned long long r = part[t];
	for (uint32_t i = b; i < e; i++) { offsets[i] = r; r += lens[i]; }
}

void launchCorrectedCount(hipStream_t stream, const DGraph& g, const OutJob* jobs, uint32_t nJobs, const LongCell* cellPool, uint32_t* lens, uint64_t* offsets, unsigned long long* total)
{
	if (!nJobs) return;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_corr_walk<false>), dim3(nJobs), dim3(64), 0, stream, g, jobs, nJobs, cellPool, lens, (const uint64_t*)nullptr, (char*)nullptr);
	hipLaunchKernelGGL(k_corr_place, dim3(1), dim3(1024), 0, stream, (const uint32_t*)lens, nJobs, offsets, total);
}

void launchCorrectedWrite(hipStream_t stream, const DGraph& g, const OutJob* jobs, uint32_t nJobs, const LongCell* cellPool, uint32_t* lens, const uint64_t* offsets, char* text)
{
	if (!nJobs) return;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_corr_walk<true>), dim3(nJobs), dim3(64), 0, stream, g, jobs, nJobs, cellPool, lens, offsets, text);
}

} // namespace gcdev
