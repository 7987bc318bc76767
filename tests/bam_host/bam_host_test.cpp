// The BAM loader's core (csrc/hip/gc_bam_core.hpp) as an ordinary program: the walk, the per-record checks and the unpacking, run on the host in the order the kernels run
// them (hip/gc_bam.hip), over the cases of a file: one per line, "<flags> <bytes in hex or ->". Prints per case "ERR <record or -1 for the header> <byte> <status>", or
// "OK <records> <consumed> <skipped>" and one line "<id in hex or -> <read or ->" per kept record. Every case's bytes lie in an allocation of exactly their length, so under
// -fsanitize=address a read past their end stops the program.
#include "gc_bam_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace gcdev;

static int hexDigit(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static void runCase(uint32_t flags, const std::string& hex)
{
	const uint32_t len = hex == "-" ? 0 : (uint32_t)(hex.size() / 2);
	uint8_t* text = (uint8_t*)malloc(len ? len : 1);
	for (uint32_t i = 0; i < len; i++) text[i] = (uint8_t)(hexDigit(hex[2 * i]) << 4 | hexDigit(hex[2 * i + 1]));
	std::vector<uint32_t> recStart;
	BamBytes rd { text };
	const BamWalk w = bamWalk(rd, len, flags, [&](uint32_t k, uint32_t start) { if (k != recStart.size()) abort(); recStart.push_back(start); });
	if (w.n != recStart.size() || w.consumed > len) abort();
	unsigned long long refused = BAM_NONE_REFUSED;
	std::vector<BamSpan> spans;
	std::vector<uint64_t> readOff { 0 };
	for (uint32_t i = 0; i < w.n; i++) {
		const BamRecord r = bamFields(text, recStart[i]);
		if (r.status != BAM_OK) { const unsigned long long key = ((unsigned long long)i << BAM_STATUS_BITS) | r.status; if (key < refused) refused = key; continue; }
		if (!r.keep) continue;
		spans.push_back(r.span);
		readOff.push_back(readOff.back() + (r.span.lSeqRev & 0x7fffffffu));
	}
	if (refused != BAM_NONE_REFUSED) printf("ERR %llu %u %llu\n", refused >> BAM_STATUS_BITS, recStart[refused >> BAM_STATUS_BITS], refused & ((1u << BAM_STATUS_BITS) - 1));
	else if (w.status != BAM_OK) printf("ERR %lld %u %u\n", w.inHeader ? -1ll : (long long)w.n, w.badAt, w.status);
	else {
		const uint32_t nKept = (uint32_t)spans.size();
		const uint64_t total = readOff.back();
		char* bases = (char*)malloc(total ? total : 1);
		memset(bases, '?', total);
		for (uint64_t p0 = 0; p0 < total; p0 += BAM_UNPACK_LETTERS) {      // one call per thread of k_bam_unpack
			const uint64_t p1 = p0 + BAM_UNPACK_LETTERS < total ? p0 + BAM_UNPACK_LETTERS : total;
			bamUnpackSpan(text, spans.data(), readOff.data(), nKept, p0, p1, [&](uint32_t k, uint8_t c) { if (bases[p0 + k] != '?') abort(); bases[p0 + k] = (char)c; });
		}
		printf("OK %u %u %u\n", w.n, w.consumed, w.n - nKept);
		for (uint32_t k = 0; k < nKept; k++) {
			const BamSpan& s = spans[k];
			if (s.nameLen == 1) printf("-");
			for (uint32_t i = 0; i + 1 < s.nameLen; i++) printf("%02x", text[s.nameAt + i]);
			printf(" ");
			if (readOff[k + 1] == readOff[k]) printf("-");
			fwrite(bases + readOff[k], 1, readOff[k + 1] - readOff[k], stdout);
			printf("\n");
		}
		free(bases);
	}
	free(text);
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: bam_host_test cases.txt\n"); return 2; }
	std::ifstream in(argv[1]);
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream fields(line);
		uint32_t flags = 0;
		std::string hex;
		if (!(fields >> flags >> hex)) { fprintf(stderr, "bad case line\n"); return 2; }
		runCase(flags, hex);
	}
	return 0;
}
