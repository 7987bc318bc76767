// csrc/hip/gc_corrected_core.hpp as an ordinary program (g++, also under -fsanitize=address,undefined): the keep rule and the letter table over 64 emulated lanes, and
// the host's record assembly. tests/test_corrected_host.py writes the cases, runs this and holds what it prints to tests/corrected_model.py.
//   T n (node offset switch) x n                 -> "T <piece>": the piece as 64 lanes per step place it (carry of the previous chunk's last cell, keep mask, rank below
//                                                   the lane), after it was found equal to the plain loop over the cells (exit 1 otherwise)
//   B maxOverlap hex(id) hex(raw) k (start end hex(piece)) x k  -> "B hex(record) hex(clipped records)"
// The graph letter of (node, offset) is corrLetter((node * 5 + offset) & 15): every entry of the table is reached.
#include "gc_corrected_core.hpp"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace gcdev;

static char letterAt(int32_t node, uint32_t offset) { return corrLetter(((uint32_t)node * 5u + offset) & 15u); }

static std::string unhex(const std::string& h)
{
	std::string out;
	if (h == "-") return out;
	for (size_t i = 0; i + 1 < h.size(); i += 2) out += (char)std::stoi(h.substr(i, 2), nullptr, 16);
	return out;
}
static std::string hex(const std::string& s)
{
	static const char* digits = "0123456789abcdef";
	std::string out;
	for (unsigned char c : s) { out += digits[c >> 4]; out += digits[c & 15]; }
	return out.empty() ? "-" : out;
}

static std::string plainLoop(const std::vector<CorrLane>& cells)   // src/GraphAligner.h:225-230 as it is written
{
	std::string out(1, letterAt(cells[0].node, cells[0].offset));
	for (size_t i = 1; i < cells.size(); i++) {
		if (!cells[i - 1].nodeSwitch && cells[i].offset == cells[i - 1].offset && cells[i].node == cells[i - 1].node) continue;
		out += letterAt(cells[i].node, cells[i].offset);
	}
	return out;
}

// the kernel's loop with the wave spelled out: a counting pass, then a writing pass into exactly that many letters
static std::string byLanes(const std::vector<CorrLane>& cells)
{
	const uint32_t n = (uint32_t)cells.size();
	std::string out;
	for (int pass = 0; pass < 2; pass++) {
		CorrLane carry { 0, 0, 0 };
		uint32_t cur = 0;
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t nValid = n - base < 64 ? n - base : 64;
			CorrLane lanes[64];
			for (uint32_t l = 0; l < 64; l++) lanes[l] = cells[base + l < n ? base + l : n - 1];   // (lanes past the end load the last cell, as the kernel does)
			const uint64_t keepMask = corrKeepMask(lanes, nValid, base, carry);
			if (pass == 1)
				for (uint32_t l = 0; l < nValid; l++)
					if ((keepMask >> l) & 1) out.at(cur + corrRank(keepMask, l)) = letterAt(lanes[l].node, lanes[l].offset);   // (.at: a place past the counted size throws)
			cur += (uint32_t)__builtin_popcountll(keepMask);
			carry = lanes[nValid - 1];
		}
		if (pass == 0) out.assign(cur, '?');
		else if (cur != out.size()) { fprintf(stderr, "the two passes disagree: %u against %zu\n", cur, out.size()); exit(1); }
	}
	return out;
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: corrected_host_test cases.txt\n"); return 2; }
	{
		const std::string table = "NACMGRSVTWYHKDBN";   // index = A | C << 1 | G << 2 | T << 3 (AlignmentGraph::NodeSequences, src/AlignmentGraph.cpp:751-796)
		for (uint32_t s = 0; s < 16; s++) if (corrLetter(s) != table[s]) { fprintf(stderr, "letter table entry %u\n", s); return 1; }
	}
	std::ifstream in(argv[1]);
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream f(line);
		std::string kind;
		f >> kind;
		if (kind == "T") {
			size_t n; f >> n;
			std::vector<CorrLane> cells(n);
			for (auto& c : cells) f >> c.node >> c.offset >> c.nodeSwitch;
			const std::string plain = plainLoop(cells), lanes = byLanes(cells);
			if (plain != lanes) { fprintf(stderr, "trace of %zu cells: the lanes give %s, the plain loop %s\n", n, lanes.c_str(), plain.c_str()); return 1; }
			std::cout << "T " << lanes << "\n";
		} else if (kind == "B") {
			size_t maxOverlap, k; std::string id, raw;
			f >> maxOverlap >> id >> raw >> k;
			id = unhex(id); raw = unhex(raw);
			std::vector<std::string> texts(k);
			std::vector<CorrPiece> pieces(k);
			for (size_t i = 0; i < k; i++) { std::string h; f >> pieces[i].start >> pieces[i].end >> h; texts[i] = unhex(h); }
			for (size_t i = 0; i < k; i++) { pieces[i].text = texts[i].data(); pieces[i].len = texts[i].size(); }
			std::string record, clipped;
			corrRecord(record, id, raw.data(), raw.size(), pieces, maxOverlap);
			for (size_t i = 0; i < k; i++) corrClippedRecord(clipped, id, i, pieces[i]);
			std::cout << "B " << hex(record) << " " << hex(clipped) << "\n";
		}
	}
	return 0;
}
