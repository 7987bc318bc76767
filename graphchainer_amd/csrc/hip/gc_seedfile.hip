// Seeds from GAM files on the device (gc_seed_store_open, gc_seeds_from_store): the kernels around gc_seedfile_core.hpp, which says what a message becomes.
//   k_sf_decode   one lane per message. The 64 messages of a wave lie back to back in the piece (the host framer gathers the messages' bytes), so the wave copies their span
//                 into its LDS tile with 16-byte loads and every lane walks its message there; a span larger than the tile (a long name, an unknown field) is walked from
//                 global memory by the same function. Hit, name hash and name span per message; an atomic minimum keeps the first message that is refused.
//   k_sf_names    the names of a piece, compacted into the store's pool (8 lanes per message)
//   sfSortStore   one stable radix sort of (hash, message): equal names end up in file order, files in command-line order
//   k_sf_join     one wave per read, in two passes (count, then gather behind a scan): the read's name is hashed, its range found by a binary search, and every candidate's
//                 NAME BYTES are compared, so two names with one hash cost time and never a wrong seed. The gather pass also makes gc_seeds_upload's two host checks.
// All of it is memory-bound with a few registers per thread; -DGC_SEEDFILE_NO_LDS compiles the staging out (every wave walks global memory), for the comparison in DESIGN.md.
#include <hip/hip_runtime.h>
#include "gc_seedfile_core.hpp"
#include <hipcub/hipcub.hpp>

namespace gcdev {

namespace {

#define SF_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

inline uint32_t sfBlocks(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

__global__ void __launch_bounds__(SF_BLOCK) k_sf_decode(const uint8_t* __restrict__ piece, const uint32_t* __restrict__ msgOff, uint32_t n, uint64_t firstMessage, uint32_t hashBits,
	SeedHit* __restrict__ hits, uint64_t* __restrict__ hash, uint32_t* __restrict__ nameStart, uint32_t* __restrict__ nameLen, unsigned long long* __restrict__ firstBad)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t sfTiles[];   // SF_WAVES tiles of SF_WAVE_TILE bytes: all of the kernel's LDS, so every tile starts at a multiple of 16
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t w0 = ((uint64_t)blockIdx.x * SF_WAVES + wave) * 64;
	const bool active = w0 < n;
	const uint32_t wEnd = active ? (uint32_t)(w0 + 64 < n ? w0 + 64 : n) : 0;
	const uint32_t spanStart = active ? msgOff[w0] : 0, spanEnd = active ? msgOff[wEnd] : 0;
	const uint32_t base = spanStart & ~15u;                               // (the piece starts at a 256-byte boundary and is padded to a multiple of 16)
#if defined(GC_SEEDFILE_NO_LDS)
	const bool staged = false;
#else
	const bool staged = active && spanEnd - base <= SF_WAVE_TILE;
	uint8_t* tile = sfTiles + wave * SF_WAVE_TILE;
	if (staged) for (uint32_t b = base + lane * 16; b < spanEnd; b += 64 * 16) *reinterpret_cast<uint4*>(tile + (b - base)) = *reinterpret_cast<const uint4*>(piece + b);
	__syncthreads();
#endif
	const uint64_t i = w0 + lane;
	if (i >= n) return;
	const uint32_t start = msgOff[i], len = msgOff[i + 1] - start;
	SfSeed s;
	uint64_t h;
#if !defined(GC_SEEDFILE_NO_LDS)
	if (staged) {
		const uint8_t* p = tile + (start - base);
		s = sfDecode(p, len);
		h = sfNameHash(p + s.nameStart, s.nameLen, hashBits);
	} else
#endif
	{
		const uint8_t* p = piece + start;
		s = sfDecode(p, len);
		h = sfNameHash(p + s.nameStart, s.nameLen, hashBits);
	}
	if (s.status != SF_OK) atomicMin(firstBad, ((unsigned long long)(firstMessage + i) << 2) | s.status);
	hits[i] = s.hit; hash[i] = h; nameStart[i] = s.nameStart; nameLen[i] = s.nameLen;
}

constexpr uint32_t SF_NAME_LANES = 8;
__global__ void __launch_bounds__(SF_BLOCK) k_sf_names(const uint8_t* __restrict__ piece, const uint32_t* __restrict__ msgOff, const uint32_t* __restrict__ nameStart, const uint32_t* __restrict__ nameLen,
	const uint32_t* __restrict__ local, uint32_t n, uint64_t poolAt, uint8_t* __restrict__ pool, uint64_t* __restrict__ nameOff)
{
	const uint64_t t = (uint64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
	const uint64_t i = t / SF_NAME_LANES;
	if (i >= n) return;
	const uint32_t sub = (uint32_t)(t % SF_NAME_LANES), len = nameLen[i];
	const uint8_t* src = piece + msgOff[i] + nameStart[i];
	uint8_t* dst = pool + poolAt + local[i];
	for (uint32_t k = sub; k < len; k += SF_NAME_LANES) dst[k] = src[k];
	if (!sub) nameOff[i] = poolAt + local[i];
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_iota(uint32_t* __restrict__ v, uint32_t n)
{
	const uint64_t i = (uint64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
	if (i < n) v[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_distinct(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ distinct)
{
	const uint64_t i = (uint64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
	const bool head = i < n && (i == 0 || sorted[i] != sorted[i - 1]);
	const uint32_t count = (uint32_t)__popcll(__ballot(head));
	if ((threadIdx.x & 63) == 0 && count) atomicAdd(distinct, count);
}

// One wave per read and one more. GATHER false: first[r] (where the name's hash begins in the sorted order) and count[r]. GATHER true: the hits in file order behind off64[r],
// readHitOff narrowed to 32 bits, and the two checks gc_seeds_upload makes on the host (match_len of 2^31 or more; match_len + read length + raw_goodness beyond 32 bits).
template <bool GATHER>
__global__ void __launch_bounds__(SF_BLOCK) k_sf_join(SfStoreView s, const uint8_t* __restrict__ names, const uint64_t* __restrict__ nameOff, uint32_t nReads, uint32_t* __restrict__ first,
	uint64_t* __restrict__ count, const uint64_t* __restrict__ off64, const uint64_t* __restrict__ readOff, SeedHit* __restrict__ out, uint32_t* __restrict__ readHitOff,
	unsigned long long* __restrict__ badLen, unsigned long long* __restrict__ badGoodness)
{
	const uint64_t r = ((uint64_t)blockIdx.x * SF_BLOCK + threadIdx.x) >> 6;
	const uint32_t lane = threadIdx.x & 63;
	if (r > nReads) return;
	if (r == nReads) {
		if (lane == 0) { if (GATHER) readHitOff[r] = (uint32_t)off64[r]; else count[r] = 0; }
		return;
	}
	const uint8_t* name = names + nameOff[r];
	const uint32_t len = (uint32_t)(nameOff[r + 1] - nameOff[r] - 1);   // (every name is followed by its terminator byte)
	uint32_t lo;
	uint64_t h, at = 0;
	if (GATHER) {
		at = off64[r];
		if (lane == 0) readHitOff[r] = (uint32_t)at;
		if (off64[r + 1] == at) return;
		lo = first[r];
		h = s.sortedHash[lo];
	} else {
		h = sfNameHash(name, len, s.hashBits);
		uint32_t hi = s.n;
		lo = 0;
		while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (s.sortedHash[mid] < h) lo = mid + 1; else hi = mid; }
	}
	uint64_t total = 0;
	uint32_t longest = 0, badAt = 0xffffffffu;
	uint64_t best = 0;   // (raw_goodness << 32) | index: the last hit among those of the largest raw_goodness
	for (uint64_t base = lo; ; base += 64) {
		const uint64_t c = base + lane;
		const bool in = c < s.n && s.sortedHash[c] == h;
		bool match = false;
		uint32_t m = 0;
		if (in) { m = s.order[c]; match = s.nameLen[m] == len && sfSameName(s.namePool + s.nameOff[m], name, len); }
		const uint64_t mask = __ballot(match);
		if (GATHER && match) {
			const uint64_t k = total + (uint64_t)__popcll(mask & ((1ull << lane) - 1));
			const SeedHit hit = s.hits[m];
			out[at + k] = hit;
			if (hit.matchLen > 0x7fffffffu && badAt == 0xffffffffu) badAt = (uint32_t)k;
			longest = hit.matchLen > longest ? hit.matchLen : longest;
			const uint64_t key = ((uint64_t)hit.rawGoodness << 32) | (uint32_t)k;
			best = key > best ? key : best;
		}
		total += (uint64_t)__popcll(mask);
		if (__ballot(in) != ~0ull) break;
	}
	if (!GATHER) {
		if (lane == 0) { first[r] = lo; count[r] = total; }
		return;
	}
	for (int d = 32; d; d >>= 1) {
		const uint32_t oLongest = __shfl_xor(longest, d), oBad = __shfl_xor(badAt, d);
		const uint64_t oBest = __shfl_xor(best, d);
		longest = oLongest > longest ? oLongest : longest;
		badAt = oBad < badAt ? oBad : badAt;
		best = oBest > best ? oBest : best;
	}
	if (lane == 0) {
		const uint64_t readLen = readOff[r + 1] - readOff[r];
		if (badAt != 0xffffffffu) atomicMin(badLen, ((unsigned long long)r << 32) | badAt);
		else if ((uint64_t)longest + readLen + (best >> 32) > 0xffffffffull) atomicMin(badGoodness, ((unsigned long long)r << 32) | (uint32_t)best);
	}
}

} // namespace

size_t sfTempBytes(uint32_t nMessages, uint32_t nReads)
{
	size_t most = 0, bytes = 0;
	if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nMessages) == hipSuccess && bytes > most) most = bytes;
	if (hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nMessages, 0, 64) == hipSuccess && bytes > most) most = bytes;
	if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)nReads + 1) == hipSuccess && bytes > most) most = bytes;
	return most + 256;
}

hipError_t sfDecodePiece(hipStream_t q, const uint8_t* piece, const uint32_t* msgOff, uint32_t nMessages, uint64_t firstMessage, uint32_t hashBits, SeedHit* hits, uint64_t* hash,
	uint32_t* nameStart, uint32_t* nameLen, unsigned long long* firstBad)
{
	if (!nMessages) return hipSuccess;
	hipLaunchKernelGGL(k_sf_decode, dim3(sfBlocks(nMessages, SF_BLOCK)), dim3(SF_BLOCK), SF_WAVES * SF_WAVE_TILE, q, piece, msgOff, nMessages, firstMessage, hashBits, hits, hash, nameStart, nameLen, firstBad);
	return hipGetLastError();
}

hipError_t sfScanNameLengths(hipStream_t q, void* temp, size_t tempBytes, const uint32_t* nameLen, uint32_t nMessages, uint32_t* nameOffLocal)
{
	if (!nMessages) return hipSuccess;
	return hipcub::DeviceScan::ExclusiveSum(temp, tempBytes, nameLen, nameOffLocal, (int)nMessages, q);
}

hipError_t sfCopyNames(hipStream_t q, const uint8_t* piece, const uint32_t* msgOff, const uint32_t* nameStart, const uint32_t* nameLen, const uint32_t* nameOffLocal, uint32_t nMessages,
	uint64_t poolAt, uint8_t* pool, uint64_t* nameOff)
{
	if (!nMessages) return hipSuccess;
	hipLaunchKernelGGL(k_sf_names, dim3(sfBlocks((uint64_t)nMessages * SF_NAME_LANES, SF_BLOCK)), dim3(SF_BLOCK), 0, q, piece, msgOff, nameStart, nameLen, nameOffLocal, nMessages, poolAt, pool, nameOff);
	return hipGetLastError();
}

// sortedHash and order from hash; iota: scratch [n]; distinct: one zeroed word
hipError_t sfSortStore(hipStream_t q, void* temp, size_t tempBytes, const uint64_t* hash, uint32_t n, uint64_t* sortedHash, uint32_t* order, uint32_t* iota, uint32_t* distinct)
{
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_sf_iota, dim3(sfBlocks(n, SF_BLOCK)), dim3(SF_BLOCK), 0, q, iota, n);
	SF_TRY(hipGetLastError());
	SF_TRY(hipcub::DeviceRadixSort::SortPairs(temp, tempBytes, hash, sortedHash, (const uint32_t*)iota, order, (int)n, 0, 64, q));
	hipLaunchKernelGGL(k_sf_distinct, dim3(sfBlocks(n, SF_BLOCK)), dim3(SF_BLOCK), 0, q, (const uint64_t*)sortedHash, n, distinct);
	return hipGetLastError();
}

hipError_t sfJoinCount(hipStream_t q, const SfStoreView& s, const uint8_t* names, const uint64_t* nameOff, uint32_t nReads, uint32_t* first, uint64_t* count)
{
	hipLaunchKernelGGL(k_sf_join<false>, dim3(sfBlocks(((uint64_t)nReads + 1) * 64, SF_BLOCK)), dim3(SF_BLOCK), 0, q, s, names, nameOff, nReads, first, count, (const uint64_t*)nullptr, (const uint64_t*)nullptr,
		(SeedHit*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
	return hipGetLastError();
}

hipError_t sfJoinScan(hipStream_t q, void* temp, size_t tempBytes, const uint64_t* count, uint32_t nReads, uint64_t* off64)
{
	return hipcub::DeviceScan::ExclusiveSum(temp, tempBytes, count, off64, (int)nReads + 1, q);
}

hipError_t sfJoinGather(hipStream_t q, const SfStoreView& s, const uint8_t* names, const uint64_t* nameOff, uint32_t nReads, const uint32_t* first, const uint64_t* off64, const uint64_t* readOff,
	SeedHit* hits, uint32_t* readHitOff, unsigned long long* badLen, unsigned long long* badGoodness)
{
	hipLaunchKernelGGL(k_sf_join<true>, dim3(sfBlocks(((uint64_t)nReads + 1) * 64, SF_BLOCK)), dim3(SF_BLOCK), 0, q, s, names, nameOff, nReads, const_cast<uint32_t*>(first), (uint64_t*)nullptr, off64, readOff,
		hits, readHitOff, badLen, badGoodness);
	return hipGetLastError();
}

} // namespace gcdev
