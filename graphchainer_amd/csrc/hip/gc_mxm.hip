// gc_seeds_mxm on the device: MUM / MEM seeds of a read batch from the suffix-array index of the graph's segments (the reference's MummerSeeder, src/MummerSeeder.cpp), as SeedHit
// records that never visit the host. The per-position logic is gc_mxm_core.hpp (it also compiles for the host: tests/mxm_host).
//   k_mxm_prefix_table   the direct-address table from the first prefixLen letters to an SA interval, from the finished suffix array: one thread per suffix writes the interval ends it sees
//   k_mxm_seed           twice over (read, strand, query position), count then fill. A wave owns a tile of 64 consecutive positions of one read and strand: one position per lane
//                        looks its interval up (prefix table, then binary search on packed words), then the wave expands the tile's intervals together, one OCCURRENCE per lane -
//                        interval sizes run from 0 to thousands on a tandem array, and a lane looping over its own interval would hold its 63 neighbours for all of it. Output
//                        slots come from the ballot of a turn and the tile's offset (a device scan of the counts between the passes).
//   k_mxm_*              the defined per-read order (matchLen descending, forward first, query position, text position: two stable radix sorts of an index permutation), the
//                        `count` longest per read, and the final records in the block layout gc_seeds_upload builds.
#include "gc_kernels.hpp"
#include "gc_mxm_core.hpp"
#include "../host/gc_layout.hpp"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace gcdev {

namespace {

__device__ __forceinline__ uint64_t prefixCodeOfSuffix(const MxmIndexView& ix, uint32_t idx)
{
	uint32_t valid;
	const uint64_t w = mxmTextWord(ix, ix.sa[idx], valid);
	return valid >= ix.prefixLen ? w >> (64 - 2 * ix.prefixLen) : ~0ull;
}

__global__ void __launch_bounds__(256) k_mxm_prefix_table(MxmIndexView ix, uint32_t* __restrict__ table)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ix.n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t idx = (uint32_t)i;
		const uint64_t code = prefixCodeOfSuffix(ix, idx);
		if (code == ~0ull) continue;
		if (idx == 0 || prefixCodeOfSuffix(ix, idx - 1) != code) table[2 * code] = idx;
		if (idx + 1 == ix.n || prefixCodeOfSuffix(ix, idx + 1) != code) table[2 * code + 1] = idx + 1;
	}
}

// tileOff[r]: the first tile of read r; a read has twice ceil(positions / 64) tiles, forward strand first (none when it is shorter than minLen or flagged invalid)
template <bool FILL>
__global__ void __launch_bounds__(256) k_mxm_seed(MxmIndexView ix, const char* __restrict__ bases, const uint64_t* __restrict__ readOff, const uint32_t* __restrict__ tileOff, uint32_t nReads, uint32_t nTiles,
	int32_t mode, uint32_t minLen, uint32_t* __restrict__ tileCount, const uint64_t* __restrict__ tileHitOff, SeedHit* __restrict__ hits, uint64_t* __restrict__ keyInner, uint64_t* __restrict__ keyOuter)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (tile >= nTiles) return;   // (whole waves leave; nothing below synchronises across waves)
	if (FILL && tileHitOff[tile + 1] == tileHitOff[tile]) return;   // most tiles of a read hold no match: the fill pass repeats the lookups only where the count pass found one
	uint32_t r = 0, hiRead = nReads - 1;   // the last read whose first tile is at or before this one (reads without tiles share their successor's first tile)
	while (r < hiRead) { const uint32_t mid = r + ((hiRead - r + 1) >> 1); if (tileOff[mid] <= tile) r = mid; else hiRead = mid - 1; }
	const uint32_t perStrand = (tileOff[r + 1] - tileOff[r]) >> 1, local = tile - tileOff[r];
	const uint32_t reverse = local >= perStrand ? 1u : 0u, firstPos = (reverse ? local - perStrand : local) * 64;
	const MxmQuery q { bases + readOff[r], (uint32_t)(readOff[r + 1] - readOff[r]), reverse };

	uint32_t lo, hi;
	(void)mxmInterval(ix, q, firstPos + lane, minLen, lo, hi);   // (false: lo = hi = 0)
	const uint32_t cnt = hi - lo;
	unsigned long long end = cnt;   // inclusive prefix sum of the tile's interval sizes (64 bits: with a tiny min_len on a large text 64 intervals exceed 2^32 suffixes)
	for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(end, d); if ((int)lane >= d) end += o; }
	const unsigned long long total = __shfl(end, 63);
	uint64_t found = 0;
	const uint64_t outBase = FILL ? tileHitOff[tile] : 0;
	for (unsigned long long base = 0; base < total; base += 64) {
		const unsigned long long item = base + lane;
		const bool active = item < total;
		uint32_t owner = 0;   // the lane whose interval holds the item: how many lanes end at or before it
		for (uint32_t step = 32; step; step >>= 1) { const unsigned long long e = __shfl(end, (int)(owner + step - 1)); if (active && e <= item) owner += step; }
		const uint32_t oLo = __shfl(lo, (int)owner), oCnt = __shfl(cnt, (int)owner);
		const unsigned long long oEnd = __shfl(end, (int)owner);
		SeedHit hit;
		uint32_t tpos = 0;
		const uint32_t pos = firstPos + owner;
		const bool ok = active && mxmOccurrence(ix, q, mode, minLen, pos, oLo, oLo + oCnt, oLo + (uint32_t)(item - (oEnd - oCnt)), hit, tpos);
		const unsigned long long ballot = __ballot(ok);
		if (FILL && ok) {
			const uint64_t slot = outBase + found + (uint64_t)__popcll(ballot & ((1ull << lane) - 1ull));
			hits[slot] = hit;
			keyInner[slot] = mxmOrderKeyInner(reverse, pos, tpos);
			keyOuter[slot] = mxmOrderKeyOuter(r, hit.matchLen);
		}
		found += (uint64_t)__popcll(ballot);
	}
	if (!FILL && lane == 0) tileCount[tile] = found > 0xffffffffull ? 0xffffffffu : (uint32_t)found;   // (saturated: the batch total is then past what the caller accepts)
}

__global__ void __launch_bounds__(256) k_mxm_iota(uint32_t* __restrict__ idx, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) idx[i] = i;
}

__global__ void __launch_bounds__(256) k_mxm_gather_keys(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t n, uint64_t* __restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = keys[idx[i]];
}

// candOff[r] = the first sorted candidate of read r (r = nReads: the total); kept[r] = how many of them stay
__global__ void __launch_bounds__(256) k_mxm_read_ranges(const uint64_t* __restrict__ sortedOuter, uint32_t n, uint32_t nReads, uint64_t maxCount, uint32_t* __restrict__ candOff, uint32_t* __restrict__ kept)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > nReads) return;
	auto firstOf = [&](uint32_t read) { uint32_t lo = 0, hi = n; while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint32_t)(sortedOuter[mid] >> 32) < read) lo = mid + 1; else hi = mid; } return lo; };
	const uint32_t a = firstOf(r);
	candOff[r] = a;
	if (r < nReads) { const uint32_t have = firstOf(r + 1) - a; kept[r] = (uint64_t)have > maxCount ? (uint32_t)maxCount : have; }
	else kept[r] = 0;
}

__global__ void __launch_bounds__(256) k_mxm_final(const SeedHit* __restrict__ cand, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ candOff, const uint64_t* __restrict__ keptOff, uint32_t nReads,
	uint64_t nFinal, SeedHit* __restrict__ out, uint32_t* __restrict__ readHitOff)
{
	const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j <= nReads) readHitOff[j] = (uint32_t)keptOff[j];
	if (j >= nFinal) return;
	uint32_t lo = 0, hi = nReads - 1;   // the read of final hit j: the first r with keptOff[r + 1] > j
	while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keptOff[mid + 1] <= j) lo = mid + 1; else hi = mid; }
	out[j] = cand[idx[candOff[lo] + (uint32_t)(j - keptOff[lo])]];
}

inline uint32_t blocksOf(uint64_t n) { return (uint32_t)((n + 255) / 256); }

} // namespace

void launchMxmPrefixTable(hipStream_t stream, const MxmIndexView& ix, uint32_t* table)
{
	if (!ix.n || !ix.prefixLen) return;
	const uint64_t blocks = ((uint64_t)ix.n + 255) / 256;
	hipLaunchKernelGGL(k_mxm_prefix_table, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, ix, table);
}

#define MXM_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t MxmSeedRun::candidates(hipStream_t q, const MxmIndexView& ix, const char* bases, const uint64_t* readOff, const uint32_t* tileOff, uint32_t nReads, uint32_t nTiles, int32_t mode, uint32_t minLen)
{
	nCandidates = 0;
	if (!nReads || !nTiles) return hipSuccess;
	// pass 1: hits per tile, then their offsets (64-bit: the batch total is checked by the caller before anything is sized by it)
	size_t scanBytes = 0;
	uint32_t* tileCount = nullptr;
	using Widen = hipcub::TransformInputIterator<uint64_t, hipcub::CastOp<uint64_t>, const uint32_t*>;
	MXM_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, Widen(tileCount, hipcub::CastOp<uint64_t>()), (uint64_t*)nullptr, (int)nTiles + 1, q));
	const size_t oCount = 0, oOff = ((size_t)(nTiles + 1) * 4 + 255) & ~(size_t)255, oTmp = oOff + (((size_t)(nTiles + 1) * 8 + 255) & ~(size_t)255);
	MXM_TRY(hipMalloc(&tiles, oTmp + scanBytes + 256));
	tileCount = (uint32_t*)((char*)tiles + oCount);
	uint64_t* tileHitOff = (uint64_t*)((char*)tiles + oOff);
	MXM_TRY(hipMemsetAsync(tileCount, 0, (size_t)(nTiles + 1) * 4, q));
	const uint32_t blocks = (nTiles + 3) / 4;
	hipLaunchKernelGGL(k_mxm_seed<false>, dim3(blocks), dim3(256), 0, q, ix, bases, readOff, tileOff, nReads, nTiles, mode, minLen, tileCount, (const uint64_t*)nullptr, (SeedHit*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
	MXM_TRY(hipGetLastError());
	MXM_TRY(hipcub::DeviceScan::ExclusiveSum((char*)tiles + oTmp, scanBytes, Widen(tileCount, hipcub::CastOp<uint64_t>()), tileHitOff, (int)nTiles + 1, q));
	MXM_TRY(hipMemcpyAsync(&nCandidates, tileHitOff + nTiles, 8, hipMemcpyDeviceToHost, q));
	MXM_TRY(hipStreamSynchronize(q));
	if (nCandidates == 0 || nCandidates > 0x7fffffffull) return hipSuccess;   // (the caller refuses the batch: hipCUB counts in int)
	// pass 2: the records and their two sort keys
	const uint64_t n = nCandidates;
	gc::Arena a;   // (n >= 1 here: no part is empty)
	const size_t oHits = a.part(n * sizeof(SeedHit)), oInner = a.part(n * 8), oOuter = a.part(n * 8), oKeysA = a.part(n * 8), oKeysB = a.part(n * 8), oIdxA = a.part(n * 4), oIdxB = a.part(n * 4);
	workBytes = a.bytes();
	MXM_TRY(hipMalloc(&work, workBytes));
	char* W = (char*)work;
	cand = (SeedHit*)(W + oHits);
	uint64_t *inner = (uint64_t*)(W + oInner), *outer = (uint64_t*)(W + oOuter), *keysA = (uint64_t*)(W + oKeysA), *keysB = (uint64_t*)(W + oKeysB);
	uint32_t *idxA = (uint32_t*)(W + oIdxA), *idxB = (uint32_t*)(W + oIdxB);
	hipLaunchKernelGGL(k_mxm_seed<true>, dim3(blocks), dim3(256), 0, q, ix, bases, readOff, tileOff, nReads, nTiles, mode, minLen, (uint32_t*)nullptr, (const uint64_t*)tileHitOff, cand, inner, outer);
	MXM_TRY(hipGetLastError());
	// the defined order: stable by (strand, query position, text position), then stable by (read, matchLen descending)
	hipLaunchKernelGGL(k_mxm_iota, dim3(blocksOf(n)), dim3(256), 0, q, idxA, (uint32_t)n);
	size_t sortBytes = 0;
	MXM_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, (const uint64_t*)inner, keysA, (const uint32_t*)idxA, idxB, (int)n, 0, 64, q));
	MXM_TRY(hipMalloc(&sortTmp, sortBytes + 256));
	MXM_TRY(hipcub::DeviceRadixSort::SortPairs(sortTmp, sortBytes, (const uint64_t*)inner, keysA, (const uint32_t*)idxA, idxB, (int)n, 0, 64, q));
	hipLaunchKernelGGL(k_mxm_gather_keys, dim3(blocksOf(n)), dim3(256), 0, q, (const uint64_t*)outer, (const uint32_t*)idxB, (uint32_t)n, keysB);
	int readBits = 1;
	while (readBits < 32 && (1ull << readBits) < nReads) readBits++;
	size_t sortBytes2 = 0;
	MXM_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes2, (const uint64_t*)keysB, keysA, (const uint32_t*)idxB, idxA, (int)n, 0, 32 + readBits, q));
	if (sortBytes2 > sortBytes) { MXM_TRY(hipStreamSynchronize(q)); MXM_TRY(hipFree(sortTmp)); sortTmp = nullptr; MXM_TRY(hipMalloc(&sortTmp, sortBytes2 + 256)); }
	MXM_TRY(hipcub::DeviceRadixSort::SortPairs(sortTmp, sortBytes2, (const uint64_t*)keysB, keysA, (const uint32_t*)idxB, idxA, (int)n, 0, 32 + readBits, q));
	sortedOuter = keysA; order = idxA;
	return hipSuccess;
}

hipError_t MxmSeedRun::select(hipStream_t q, uint32_t nReads, uint64_t maxCount, uint64_t& nFinal)
{
	nFinal = 0;
	if (!nReads || !nCandidates) return hipSuccess;
	size_t scanBytes = 0;
	using Widen = hipcub::TransformInputIterator<uint64_t, hipcub::CastOp<uint64_t>, const uint32_t*>;
	MXM_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, Widen((const uint32_t*)nullptr, hipcub::CastOp<uint64_t>()), (uint64_t*)nullptr, (int)nReads + 1, q));
	const size_t slot4 = ((size_t)(nReads + 1) * 4 + 255) & ~(size_t)255, slot8 = ((size_t)(nReads + 1) * 8 + 255) & ~(size_t)255;
	MXM_TRY(hipMalloc(&ranges, 2 * slot4 + slot8 + scanBytes + 256));
	candOff = (uint32_t*)ranges;
	uint32_t* kept = (uint32_t*)((char*)ranges + slot4);
	keptOff = (uint64_t*)((char*)ranges + 2 * slot4);
	hipLaunchKernelGGL(k_mxm_read_ranges, dim3(blocksOf((uint64_t)nReads + 1)), dim3(256), 0, q, (const uint64_t*)sortedOuter, (uint32_t)nCandidates, nReads, maxCount, candOff, kept);
	MXM_TRY(hipGetLastError());
	MXM_TRY(hipcub::DeviceScan::ExclusiveSum((char*)ranges + 2 * slot4 + slot8, scanBytes, Widen((const uint32_t*)kept, hipcub::CastOp<uint64_t>()), keptOff, (int)nReads + 1, q));
	MXM_TRY(hipMemcpyAsync(&nFinal, keptOff + nReads, 8, hipMemcpyDeviceToHost, q));
	MXM_TRY(hipStreamSynchronize(q));
	return hipSuccess;
}

hipError_t MxmSeedRun::write(hipStream_t q, uint32_t nReads, uint64_t nFinal, SeedHit* out, uint32_t* readHitOff)
{
	if (!nReads) return hipSuccess;
	if (!nCandidates) return hipMemsetAsync(readHitOff, 0, (size_t)(nReads + 1) * 4, q);
	const uint64_t threads = nFinal > (uint64_t)nReads + 1 ? nFinal : (uint64_t)nReads + 1;
	hipLaunchKernelGGL(k_mxm_final, dim3(blocksOf(threads)), dim3(256), 0, q, (const SeedHit*)cand, (const uint32_t*)order, (const uint32_t*)candOff, (const uint64_t*)keptOff, nReads, nFinal, out, readHitOff);
	return hipGetLastError();
}

MxmSeedRun::~MxmSeedRun()
{
	for (void* p : { tiles, work, sortTmp, ranges }) if (p) (void)hipFree(p);
}

} // namespace gcdev
