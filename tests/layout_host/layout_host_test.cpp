// csrc/host/gc_layout.hpp on the CPU (tests/test_layout_host.py): every per-read value, every offset and the block size of the read and seed batch layouts.
// Input lines: "reads <len> <len> ..." (none: an empty batch) or "seeds <nReads> <nHits>". Output per case, one line of numbers:
//   reads: n, then per read maskOff maskWords eqOff readOff eqOff len words, then totalWords eqWords, the twelve offsets, blockBytes
//   seeds: oOff oArrays oBad oHits blockBytes
#include "gc_layout.hpp"
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

int main(int argc, char** argv)
{
	if (argc != 2) return 2;
	std::ifstream in(argv[1]);
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream words(line);
		std::string kind;
		words >> kind;
		if (kind == "reads") {
			std::vector<uint64_t> offsets { 0 };
			for (uint64_t len; words >> len;) offsets.push_back(offsets.back() + len);
			const uint64_t n = offsets.size() - 1;
			const gc::ReadBatchLayout L(offsets.data(), n);
			if (L.maskOff.size() != n || L.maskWords.size() != n || L.eqOff.size() != n || L.edReads.size() != n) return 3;
			printf("%llu", (unsigned long long)n);
			for (uint64_t r = 0; r < n; r++)
				printf(" %llu %u %llu %llu %llu %u %u", (unsigned long long)L.maskOff[r], L.maskWords[r], (unsigned long long)L.eqOff[r], (unsigned long long)L.edReads[r].readOff,
					(unsigned long long)L.edReads[r].eqOff, L.edReads[r].len, L.edReads[r].words);
			printf(" %llu %llu", (unsigned long long)L.totalWords, (unsigned long long)L.eqWords);
			for (size_t o : { L.oBases, L.oOffsets, L.oMasks, L.oEqMasks, L.oEdReads, L.oPacked, L.oInvalid, L.oChunkRead, L.oMaskOff, L.oMaskWords, L.oEqOff, L.oReadInvalid, L.blockBytes }) printf(" %zu", o);
			printf("\n");
		} else if (kind == "seeds") {
			uint64_t nReads = 0, nHits = 0;
			words >> nReads >> nHits;
			const gc::SeedBatchLayout L(nReads, nHits);
			printf("%zu %zu %zu %zu %zu\n", L.oOff, L.oArrays, L.oBad, L.oHits, L.blockBytes);
		} else return 4;
	}
	return 0;
}
