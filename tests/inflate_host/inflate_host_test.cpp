// csrc/hip/gc_inflate_core.hpp on the host (tests/test_inflate_host.py): every line of the input file is a BGZF file in hex; its whole blocks are inflated as the kernel
// inflates them (infHeader, infBlock, the CRC-32 by 64 slices). Each block's deflate data and its output lie in allocations of exactly their lengths, so that under
// -fsanitize=address a read or write past either stops the program.
// Output per line: "OK <consumed> <hex of the text>", or "ERR <block> <status>" for the first bad block.
#include "gc_inflate_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace gcdev;

static std::vector<uint8_t> unhex(const std::string& s)
{
	std::vector<uint8_t> out;
	if (s == "-") return out;
	auto v = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
	for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)(v(s[i]) << 4 | v(s[i + 1])));
	return out;
}

int main(int argc, char** argv)
{
	if (argc != 2) return 2;
	std::ifstream in(argv[1]);
	std::string line, text;
	uint32_t crcTable[256];
	for (uint32_t i = 0; i < 256; i++) crcTable[i] = infCrcTableEntry(i);
	InfTables* tables = new InfTables;
	while (std::getline(in, line)) {
		const std::vector<uint8_t> file = unhex(line);
		uint64_t at = 0, block = 0;
		uint32_t bad = INF_OK;
		text.clear();
		for (;; block++) {
			InfBlock b;
			uint32_t size = 0;
			uint8_t* member = (uint8_t*)malloc(file.size() - at ? file.size() - at : 1);
			memcpy(member, file.data() + at, file.size() - at);
			const int32_t kind = infHeader(member, file.size() - at, b, size);
			if (kind != INF_FRAME_BLOCK) { free(member); break; }
			uint8_t* cdata = (uint8_t*)malloc(b.inLen ? b.inLen : 1);
			memcpy(cdata, member + b.inOff, b.inLen);
			free(member);
			uint8_t* out = (uint8_t*)malloc(b.isize ? b.isize : 1);
			InfHostSink sink { out };
			bad = infBlock(b.inLen ? cdata : nullptr, b.inLen, b.isize, *tables, sink);
			if (!bad) {
				uint32_t crc = 0;
				for (uint32_t lane = 0; lane < INF_LANES; lane++) crc ^= infCrcLane(crcTable, b.isize ? out : nullptr, b.isize, lane, INF_LANES);
				if (crc != b.crc) bad = INF_CRC;
			}
			if (!bad) {
				static const char digits[] = "0123456789abcdef";
				for (uint32_t k = 0; k < b.isize; k++) { text.push_back(digits[out[k] >> 4]); text.push_back(digits[out[k] & 15]); }
			}
			free(cdata); free(out);
			if (bad) break;
			at += size;
		}
		if (bad) printf("ERR %llu %u\n", (unsigned long long)block, bad);
		else printf("OK %llu %s\n", (unsigned long long)at, text.empty() ? "-" : text.c_str());
	}
	delete tables;
	return 0;
}
