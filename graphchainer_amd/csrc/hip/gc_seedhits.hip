// k_seed_resolve: a host's own seed hits (SeedHit records as a seeder hands them over, src/GraphAlignerWrapper.h:14 - from a seeds file, a MEM seeder, or a filter behind getSeeds)
// become what the seed glue starts from: split node, offset in it, read position, matchLen, raw goodness, in the caller's order. One hit per lane; the per-hit function is
// gc_seedhits_core.hpp (it also compiles for the host: tests/seedhits_host). A hit that a later kernel would read out of bounds through - no such node, an offset beyond the
// original node, a read position beyond the read - is not resolved and not clamped: the smallest index of such a hit comes back and gc_seeds_upload refuses the batch.
#include "gc_kernels.hpp"
#include "gc_seedhits_core.hpp"

namespace gcdev {

__global__ void __launch_bounds__(256) k_seed_resolve(SeedLookup lookup, const SeedHit* __restrict__ hits, uint64_t nHits, const uint32_t* __restrict__ readHitOff, uint32_t nReads, const uint64_t* __restrict__ readOff,
	SeedHitArrays out, unsigned long long* __restrict__ firstBad)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nHits; i += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t lo = 0, hi = nReads - 1;   // the read of hit i: the first r with readHitOff[r + 1] > i (readHitOff[nReads] = nHits > i)
		while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (readHitOff[mid + 1] <= i) lo = mid + 1; else hi = mid; }
		const uint32_t readLen = (uint32_t)(readOff[lo + 1] - readOff[lo]);
		const SeedHit h = hits[i];
		uint32_t node = 0, offset = 0;
		const uint32_t status = seedHitResolve(lookup, h, readLen, node, offset);
		if (status != SEED_HIT_OK) atomicMin(firstBad, ((unsigned long long)i << 2) | status);
		out.node[i] = node; out.offset[i] = offset; out.seqPos[i] = h.seqPos; out.matchLen[i] = h.matchLen; out.raw[i] = h.rawGoodness;
	}
}

void launchSeedResolve(hipStream_t stream, const SeedLookup& lookup, const SeedHit* hits, uint64_t nHits, const uint32_t* readHitOff, uint32_t nReads, const uint64_t* readOff, const SeedHitArrays& out,
	unsigned long long* firstBad)
{
	if (!nHits || !nReads) return;
	const uint64_t blocks = (nHits + 255) / 256;
	hipLaunchKernelGGL(k_seed_resolve, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, lookup, hits, nHits, readHitOff, nReads, readOff, out, firstBad);
}

} // namespace gcdev
