// Where the arrays of a read batch (gc_reads) and of a seed batch (gc_seeds) lie inside their one device block, and the arena every carved block of the library is cut
// with. Arithmetic only: the blocks themselves, and the binding of a handle to one, are gc_runtime.hpp's. Standard library only: tests/layout_host builds it without HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gc {

// parts of one block, each starting on a 256-byte boundary; an empty part still takes 256 bytes, so no two parts share an address
struct Arena {
	size_t part(size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; }
	size_t bytes() const { return at; }
	size_t at = 0;
};

struct EdReadRecord { uint64_t readOff, eqOff; uint32_t len, words; };   // the kernels' EdRead (hip/gc_kernels.hpp), field for field
constexpr size_t SEED_HIT_BYTES = 24;                                      // sizeof(SeedHit) (hip/gc_seedhits_core.hpp) = sizeof(gc_seed_hit)

// A read batch from its offsets [n + 1]: the per-read layout of the bit vectors (O(n); everything per base is derived on the device from one copy of the raw bases) and
// the twelve parts of the device block
struct ReadBatchLayout {
	std::vector<uint64_t> maskOff, eqOff; std::vector<uint32_t> maskWords; std::vector<EdReadRecord> edReads;   // [n] each, what gc_reads (gc_runtime.hpp) says of them
	uint64_t totalWords = 0, eqWords = 0;
	size_t oBases, oOffsets, oMasks, oEqMasks, oEdReads, oPacked, oInvalid, oChunkRead, oMaskOff, oMaskWords, oEqOff, oReadInvalid, blockBytes;

	ReadBatchLayout(const uint64_t* offsets, uint64_t n) : maskOff(n), eqOff(n), maskWords(n), edReads(n)
	{
		for (uint64_t r = 0; r < n; r++) {
			maskOff[r] = totalWords;
			maskWords[r] = (uint32_t)((offsets[r + 1] - offsets[r] + 63) / 64 + 1);
			totalWords += 8ull * maskWords[r];
			edReads[r] = EdReadRecord { offsets[r], eqWords, (uint32_t)(offsets[r + 1] - offsets[r]), maskWords[r] };
			eqOff[r] = eqWords;
			eqWords += 4ull * maskWords[r];
		}
		const uint64_t total = offsets[n];
		Arena a;
		oBases = a.part(2 * total); oOffsets = a.part((n + 1) * sizeof(uint64_t)); oMasks = a.part(totalWords * sizeof(uint64_t)); oEqMasks = a.part(eqWords * sizeof(uint64_t));
		oEdReads = a.part(n * sizeof(EdReadRecord)); oPacked = a.part(((total >> 5) + 1) * sizeof(uint64_t)); oInvalid = a.part(((total >> 6) + 1) * sizeof(uint64_t));
		oChunkRead = a.part(((total >> 6) + 1) * sizeof(uint32_t)); oMaskOff = a.part(n * sizeof(uint64_t)); oMaskWords = a.part(n * sizeof(uint32_t)); oEqOff = a.part(n * sizeof(uint64_t));
		oReadInvalid = a.part(n);
		blockBytes = a.bytes();
	}
};

// A seed batch: the reads' hit offsets, the five resolved arrays of nHits words each, the words the kernels leave their first refused hit in (resolve, match_len,
// raw_goodness: gc_seeds_from_store uses all three, the other producers the first), and the raw records in the block's tail (24 B per hit beside the 20 B the glue reads)
struct SeedBatchLayout {
	size_t oOff, oArrays, oBad, oHits, blockBytes;
	SeedBatchLayout(uint64_t nReads, uint64_t nHits)
	{
		Arena a;
		oOff = a.part((nReads + 1) * sizeof(uint32_t)); oArrays = a.part(5 * nHits * sizeof(uint32_t)); oBad = a.part(3 * sizeof(unsigned long long)); oHits = a.part(nHits * SEED_HIT_BYTES);
		blockBytes = a.bytes();
	}
};

} // namespace gc
