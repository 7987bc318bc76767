// The seeds-file reader without a GPU: csrc/host/gc_seedfile_frame.hpp (the framer the library runs on the host) and csrc/hip/gc_seedfile_core.hpp (what every lane of
// k_sf_decode runs) as an ordinary program. Input: one case per line, "<piece bytes> <feed bytes> <hex of the inflated stream, or ->": the stream is pushed into the framer
// <feed bytes> at a time (0: all at once). Every message is decoded from an allocation of exactly its length, so a read past its end stops a sanitizer build.
// Output per case: "ERR <FRAME|MAPPING|EDIT|PARSE> <text>", or "OK <n> <pieces>" and n lines "<name hex or -> node_id node_offset seq_pos match_len raw_goodness reverse hash".
#include "gc_seedfile_core.hpp"
#include "gc_seedfile_frame.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

static std::vector<uint8_t> unhex(const std::string& h)
{
	std::vector<uint8_t> out;
	if (h == "-") return out;
	auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
	for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(v(h[i]) * 16 + v(h[i + 1])));
	return out;
}

int main(int argc, char** argv)
{
	if (argc != 2) return 2;
	std::ifstream in(argv[1]);
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream fields(line);
		size_t pieceBytes = 0, feed = 0;
		std::string hex;
		fields >> pieceBytes >> feed >> hex;
		const std::vector<uint8_t> bytes = unhex(hex);
		std::unique_ptr<uint8_t[]> stream(new uint8_t[bytes.size()]);   // (exactly its length)
		if (!bytes.empty()) memcpy(stream.get(), bytes.data(), bytes.size());
		std::ostringstream rows;
		std::string error;
		uint64_t n = 0, pieces = 0, expectFirst = 0;
		gc::SeedFileFramer framer(pieceBytes, [&](const uint8_t* data, size_t len, const uint32_t* off, uint32_t count, uint64_t first) {
			pieces++;
			if (first != expectFirst || off[0] != 0 || off[count] != len) { error = "FRAME the piece's table is inconsistent"; return; }
			expectFirst += count;
			for (uint32_t i = 0; i < count && error.empty(); i++) {
				const uint32_t mlen = off[i + 1] - off[i];
				std::unique_ptr<uint8_t[]> message(new uint8_t[mlen]);
				memcpy(message.get(), data + off[i], mlen);
				const gcdev::SfSeed s = gcdev::sfDecode(message.get(), mlen);
				if (s.status != gcdev::SF_OK) {
					const char* what[] = { "", "MAPPING", "EDIT", "PARSE" };
					error = std::string(what[s.status]) + " message " + std::to_string(n);
					return;
				}
				if ((uint64_t)s.nameStart + s.nameLen > mlen) { error = "PARSE the name lies outside the message"; return; }
				if (!s.nameLen) rows << "-";
				for (uint32_t k = 0; k < s.nameLen; k++) { char b[3]; snprintf(b, sizeof(b), "%02x", message[s.nameStart + k]); rows << b; }
				rows << " " << s.hit.nodeId << " " << s.hit.nodeOffset << " " << s.hit.seqPos << " " << s.hit.matchLen << " " << s.hit.rawGoodness << " " << s.hit.reverse << " "
					<< gcdev::sfNameHash(message.get() + s.nameStart, s.nameLen, 64) << "\n";
				n++;
			}
		});
		try {
			const size_t step = feed ? feed : std::max<size_t>(bytes.size(), 1);
			for (size_t at = 0; at < bytes.size() && error.empty(); at += step) framer.push(stream.get() + at, std::min(step, bytes.size() - at));
			if (error.empty()) framer.finish();
		} catch (const gc::SeedFileError& e) {
			if (error.empty()) error = std::string("FRAME ") + e.what();
		}
		if (error.empty() && framer.seeds() != n) error = "FRAME the framer counted other messages than it handed on";
		if (!error.empty()) std::cout << "ERR " << error << "\n";
		else std::cout << "OK " << n << " " << pieces << "\n" << rows.str();
	}
	return 0;
}
