// The minimizer seed lookup (K1) for gfx950 (MI355X). See gc_device.hpp for the device data model and DESIGN.md for the mapping rationale.
#include "gc_kernels.hpp"

namespace gcdev {

// =====================================================================================================
// K1 - minimizer seed lookup. reference: MinimizerSeeder::getSeeds / iterateKmers,
// src/MinimizerSeeder.cpp:59-102,522-544. One wave per read; lanes sweep 64 read positions at a time.
// For every read position whose 15-mer is valid and indexed with count < maxCount, and that passes the
// reference's "same k-mer as the previous position" thinning rule (:91), emits (pos, keyIndex).
// Output order inside a read is by position (ballot-rank compaction), which the host's std::sort by count
// then consumes exactly like the reference does (:497).
// =====================================================================================================

__device__ __forceinline__ int baseCode(uint8_t c)
{
	switch (c) {
		case 'a': case 'A': return 0;
		case 'c': case 'C': return 1;
		case 'g': case 'G': return 2;
		case 't': case 'T': return 3;
	}
	return -1;
}

__device__ __forceinline__ uint32_t hashKmer(uint64_t kmer)
{
	kmer *= 0x9E3779B97F4A7C15ull;
	return (uint32_t)(kmer >> 32);
}

// 9 of 10 read k-mers are not graph minimizers; a probe of the 0.1-0.5 GB table is a random HBM access each, a bit of the
// 32 MB filter is a cache hit. A clear bit proves the k-mer is not a key (a set bit proves nothing: ~2 % false positives).
__device__ __forceinline__ uint32_t filterBit(uint64_t kmer, uint32_t shift) { return (uint32_t)((kmer * 0xD6E8FEB86659FD93ull) >> shift); }

// returns key index or 0xffffffff. Open addressing, linear probing; slot = {kmer:32, index:32}.
__device__ __forceinline__ uint32_t lookupKmer(const SeedIndex& idx, uint64_t kmer)
{
	const uint32_t fb = filterBit(kmer, idx.filterShift);
	if (!((idx.filter[fb >> 5] >> (fb & 31)) & 1u)) return 0xffffffffu;
	uint32_t h = hashKmer(kmer) & idx.tableMask;
	while (true) {
		uint64_t slot = idx.table[h];
		if (slot == ~0ull) return 0xffffffffu;
		if ((uint32_t)(slot >> 32) == (uint32_t)kmer && (!idx.wideKmers || idx.wideKmers[(uint32_t)slot] == kmer)) return (uint32_t)slot;
		h = (h + 1) & idx.tableMask;
	}
}

// K1a: one thread per read base. For the k-mer that ends at the base: the reference's thinning rule, the index probe and the
// frequency cut; writes key index + 1 (0 = nothing to emit) into tmp[global position].
__global__ void __launch_bounds__(256) k_seed_probe(SeedIndex idx, const char* __restrict__ bases, const uint64_t* __restrict__ readOff, const uint32_t* __restrict__ chunkRead, const uint64_t* __restrict__ packed, const uint64_t* __restrict__ invalid, uint32_t nReads, uint64_t totalBases, uint32_t* __restrict__ tmp)
{
	const int k = idx.k;
	const int realWindow = idx.w - idx.k + 1;
	const uint64_t mask = ~(~0ull << (2 * k));
	for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < totalBases; p += (uint64_t)gridDim.x * blockDim.x) {
		// the read this base belongs to: last r with readOff[r] <= p (chunkRead: the read of the first base of every 64-base chunk)
		uint32_t lo = chunkRead[p >> 6];
		while (lo + 1 < nReads && readOff[lo + 1] <= p) lo++;
		const char* seq = bases + readOff[lo];
		const int pos = (int)(p - readOff[lo]);
		uint32_t found = 0;
		if (pos >= k - 1) {
			// k-mer ending at pos, from the 2-bit big-endian packing of the concatenated reads (base j in bits 63-2(j%32), 62-2(j%32)
			// of word j/32): the k bases are one bit field of a two-word window; a second bit vector marks the non-ACGT bases
			const uint64_t w = p >> 5;
			const uint64_t lo64 = packed[w], hi64 = w ? packed[w - 1] : 0ull;
			const uint32_t sh = 2u * (31u - (uint32_t)(p & 31));
			const uint64_t kmer = (sh ? ((lo64 >> sh) | (hi64 << (64 - sh))) : lo64) & mask;
			const uint64_t iw = p >> 6;
			const uint64_t ilo = invalid[iw], ihi = iw ? invalid[iw - 1] : 0ull;
			const uint32_t ish = 63u - (uint32_t)(p & 63);   // same big-endian convention: base j in bit 63-(j%64)
			const uint64_t window = ish ? ((ilo >> ish) | (ihi << (64 - ish))) : ilo;
			const bool valid = (window & ((1ull << k) - 1)) == 0;
			if (valid) {
				// thinning (:91): inside a streak of identical consecutive k-mers only every realWindow-th is emitted.
				// Consecutive k-mers are identical only in a homopolymer; walk back to the streak start.
				int streakStart = pos;
				int c0 = baseCode((uint8_t)seq[pos]);
				bool homopolymer = (kmer == (uint64_t)c0 * (mask / 3));
				if (homopolymer) {
					while (streakStart - k >= 0 && baseCode((uint8_t)seq[streakStart - k]) == c0) streakStart--;
				}
				bool emit = ((pos - streakStart) % realWindow) == 0;
				if (emit) {
					uint32_t key = lookupKmer(idx, kmer);
					if (key != 0xffffffffu) {
						uint32_t count = (uint32_t)(idx.startPos[key + 1] - idx.startPos[key]);
						if (count < idx.maxCount) found = key + 1;
					}
				}
			}
		}
		tmp[p] = found;
	}
}

// K1b: one wave per read: counts the read's hits, reserves a contiguous output range and compacts them in position order.
__global__ void __launch_bounds__(64) k_seed_compact(const uint64_t* __restrict__ readOff, uint32_t nReads, const uint32_t* __restrict__ tmp,
	uint64_t* __restrict__ matchCursor, uint32_t* __restrict__ readMatchOff, uint32_t* __restrict__ readMatchCount, uint2* __restrict__ matches, uint64_t matchCapacity)
{
	const int lane = threadIdx.x;
	for (uint32_t r = blockIdx.x; r < nReads; r += gridDim.x) {
		const int len = (int)(readOff[r + 1] - readOff[r]);
		const uint32_t* mine = tmp + readOff[r];
		uint32_t total = 0;
		for (int base = 0; base < len; base += 64) {
			int pos = base + lane;
			total += (uint32_t)__popcll(__ballot(pos < len && mine[pos] != 0));
		}
		// reserve a contiguous output range for this read
		uint64_t outBase = 0;
		if (lane == 0) outBase = atomicAdd((unsigned long long*)matchCursor, (unsigned long long)total);
		outBase = __shfl(outBase, 0);
		if (lane == 0) { readMatchOff[r] = (uint32_t)outBase; readMatchCount[r] = total; }
		if (outBase + total > matchCapacity) continue;   // host checks the cursor and retries with a larger buffer
		uint32_t written = 0;
		for (int base = 0; base < len; base += 64) {
			int pos = base + lane;
			uint32_t found = pos < len ? mine[pos] : 0;
			unsigned long long ballot = __ballot(found != 0);
			if (found) {
				uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
				matches[outBase + written + rank] = make_uint2((uint32_t)pos, found - 1);
			}
			written += (uint32_t)__popcll(ballot);
		}
	}
}

// =====================================================================================================
// launchers
// =====================================================================================================

void launchSeedLookup(hipStream_t stream, const SeedIndex& idx, const char* bases, const uint64_t* readOff, uint32_t nReads,
	uint64_t* matchCursor, uint32_t* readMatchOff, uint32_t* readMatchCount, uint2* matches, uint64_t matchCapacity, uint32_t* tmp, uint64_t totalBases, const uint32_t* chunkRead, const uint64_t* packed, const uint64_t* invalid)
{
	if (nReads == 0) return;
	uint64_t probeBlocks = (totalBases + 255) / 256;
	if (probeBlocks > 65536) probeBlocks = 65536;
	if (probeBlocks) hipLaunchKernelGGL(k_seed_probe, dim3((uint32_t)probeBlocks), dim3(256), 0, stream, idx, bases, readOff, chunkRead, packed, invalid, nReads, totalBases, tmp);
	uint32_t blocks = nReads < 16384 ? nReads : 16384;
	hipLaunchKernelGGL(k_seed_compact, dim3(blocks), dim3(64), 0, stream, readOff, nReads, tmp, matchCursor, readMatchOff, readMatchCount, matches, matchCapacity);
}

} // namespace gcdev
