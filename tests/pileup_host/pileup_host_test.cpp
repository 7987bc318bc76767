// csrc/hip/gc_pileup_core.hpp as an ordinary program (g++, also under -fsanitize=address,undefined): the cell kinds, the channels with the letter table and the
// complement, over 64 emulated lanes with the predecessor of lane 0 carried from the chunk before, as k_cov_add takes a trace; then the filter and the lines of the table,
// each written into exactly the bytes its length function counted. tests/test_pileup_host.py writes the cases, runs this and holds what it prints to tests/pileup_model.py.
//   G n (hex(letters) hex(name)) x n      the graph's segments in internal order, forward letters ("-": no name)
//   T n hex(read) (node offset seqPos) x n   one trace with its read, added to the accumulators
//   E minAlt minFraction first count      -> "P hex(pileup table of that range)", or "BAD" when a cell's seqPos lay behind its read (it was not counted)
//   Z                                     the accumulators back to zero
// Before a table is printed the rows must equal the plain loop's over the same cells, and depth = matches + mismatches + deletions must hold at every base (exit 1 otherwise).
#include "gc_pileup_core.hpp"
#include "gc_corrected_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace gcdev;

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
static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(1); }

static uint8_t iupac[256];
static void buildIupac()   // the library's table (gc_runtime.hpp): a byte that is no nucleotide code has the empty set
{
	memset(iupac, 0, sizeof iupac);
	auto set = [&](const char* chars, uint8_t m) { for (const char* c = chars; *c; c++) iupac[(uint8_t)*c] = m; };
	set("Aa", 1); set("Cc", 2); set("Gg", 4); set("TtUu", 8);
	set("Rr", 1 | 4); set("Yy", 2 | 8); set("Kk", 4 | 8); set("Mm", 1 | 2); set("Ss", 2 | 4); set("Ww", 1 | 8);
	set("Bb", 2 | 4 | 8); set("Dd", 1 | 4 | 8); set("Hh", 1 | 2 | 8); set("Vv", 1 | 2 | 4); set("Nn", 15);
}

struct Graph {
	std::vector<std::string> names, letters;
	std::vector<uint64_t> segStart;
	uint32_t forwardSet(uint64_t s, uint64_t pos) const { const uint32_t m = iupac[(uint8_t)letters.at(s).at(pos)]; return m ? m : 15u; }
	uint32_t setUnder(int32_t node, uint32_t offset) const
	{
		const uint64_t s = (uint32_t)node >> 1, length = segStart.at(s + 1) - segStart.at(s);
		const uint32_t m = forwardSet(s, covForward(node, offset, (uint32_t)length));
		return (node & 1) ? ((m & 1u) << 3 | (m & 2u) << 1 | (m & 4u) >> 1 | (m & 8u) >> 3) : m;
	}
};
struct Counts { std::vector<uint32_t> depth, rows, plain; bool bad = false; };

// the kernel's loop with the wave spelled out
static void addByLanes(const Graph& g, const std::vector<PileLane>& cells, const std::string& read, Counts& c)
{
	const uint32_t n = (uint32_t)cells.size();
	PileLane carry { 0, 0, 0 };
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t nValid = n - base < 64 ? n - base : 64;
		PileLane lanes[64];
		for (uint32_t l = 0; l < 64; l++) lanes[l] = cells[base + l < n ? base + l : n - 1];   // (lanes past the end load the last cell, as the kernel does)
		uint32_t channel[64];
		for (uint32_t l = 0; l < 64; l++) channel[l] = 0xdeadbeefu;
		pileChunk(lanes, nValid, base, carry, (const uint8_t*)read.data(), (uint32_t)read.size(), [&](uint8_t letter) { return (uint32_t)iupac[letter]; },
			[&](int32_t node, uint32_t offset) { return g.setUnder(node, offset); }, channel, &c.bad);
		for (uint32_t l = 0; l < nValid; l++) {
			const PileLane& p = l == 0 ? carry : lanes[l - 1];
			const uint32_t seg = covSegment(lanes[l].node);
			const uint64_t length = g.segStart.at(seg + 1) - g.segStart.at(seg);
			if (lanes[l].offset >= length) die("a cell outside its segment");
			const uint64_t at = g.segStart[seg] + covForward(lanes[l].node, lanes[l].offset, (uint32_t)length);
			if (covCovers(base + l == 0, p.node, p.offset, lanes[l].node, lanes[l].offset)) c.depth.at(at)++;
			if (channel[l] == PILE_NONE) continue;
			if (channel[l] >= PILE_CHANNELS) die("no such channel");
			c.rows.at(at * PILE_CHANNELS + channel[l])++;
		}
		carry = lanes[nValid - 1];
	}
	// the rule as it is stated, cell by cell
	for (uint32_t i = 0; i < n; i++) {
		const bool covers = i == 0 || cells[i].node != cells[i - 1].node || cells[i].offset != cells[i - 1].offset;
		const bool moved = i == 0 || cells[i].seqPos != cells[i - 1].seqPos;
		if (cells[i].seqPos >= read.size() || (!covers && !moved)) continue;
		const uint32_t seg = (uint32_t)cells[i].node >> 1;
		const uint64_t length = g.segStart[seg + 1] - g.segStart[seg];
		const bool odd = cells[i].node & 1;
		const uint64_t at = g.segStart[seg] + (odd ? length - 1 - cells[i].offset : cells[i].offset);
		const uint8_t letter = (uint8_t)read[cells[i].seqPos];
		uint32_t ch;
		if (covers && moved) {
			if (iupac[letter] & g.setUnder(cells[i].node, cells[i].offset)) continue;
			switch (letter) { case 'A': case 'a': ch = 0; break; case 'C': case 'c': ch = 1; break; case 'G': case 'g': ch = 2; break; case 'T': case 't': case 'U': case 'u': ch = 3; break; default: ch = 4; }
			if (odd && ch < 4) ch = 3 - ch;
		} else if (covers) ch = 5;
		else ch = odd ? 7 : 6;
		c.plain.at(at * 8 + ch)++;
	}
}

static std::string pileupTable(const Graph& g, const Counts& c, uint64_t first, uint64_t count, uint64_t minAlt, double minFraction)
{
	const uint64_t nSeg = g.segStart.size() - 1, nBases = g.segStart[nSeg];
	std::string out = first == 0 ? "#segment\tpos\tref\tdepth\tmatch\tmmA\tmmC\tmmG\tmmT\tmmN\tdel\tins_before\tins_after\n" : "";
	for (uint64_t i = first; i < first + count && i < nBases; i++) {
		const uint32_t* row = c.rows.data() + i * PILE_CHANNELS;
		if (!pilePasses(c.depth[i], row, minAlt, minFraction)) continue;
		const uint64_t s = covSegmentOfBase(g.segStart.data(), nSeg, i), s0 = g.segStart[s];
		const std::string& name = g.names[s];
		std::vector<char> line(pileLineLen((uint32_t)name.size(), s, i - s0, c.depth[i], row));   // exactly the counted bytes: a longer line is the sanitizer's to find
		if (pileLine(line.data(), name.data(), (uint32_t)name.size(), s, i - s0, corrLetter(g.forwardSet(s, i - s0)), c.depth[i], row) != line.size()) die("a pileup line is not as long as it was counted");
		out.append(line.data(), line.size());
	}
	return out;
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: pileup_host_test cases.txt\n"); return 2; }
	buildIupac();
	{
		// the letter table, the complement and the kinds
		for (int b = 0; b < 256; b++) {
			uint32_t want = PILE_MM_N;
			if (b == 'A' || b == 'a') want = PILE_MM_A; else if (b == 'C' || b == 'c') want = PILE_MM_C; else if (b == 'G' || b == 'g') want = PILE_MM_G;
			else if (b == 'T' || b == 't' || b == 'U' || b == 'u') want = PILE_MM_T;
			if (pileChannel((uint8_t)b, false) != want || pileChannel((uint8_t)b, true) != (want < 4 ? 3 - want : want)) die("the letter table");
		}
		if (pileKind(true, true) != PILE_KIND_PAIR || pileKind(true, false) != PILE_KIND_DELETION || pileKind(false, true) != PILE_KIND_INSERTION || pileKind(false, false) != PILE_KIND_NOTHING) die("the kinds");
		if (pileCellChannel(PILE_KIND_INSERTION, false, 'A', 1, 1) != PILE_INS_AFTER || pileCellChannel(PILE_KIND_INSERTION, true, 'A', 1, 1) != PILE_INS_BEFORE) die("the insertion channels");
		// a full word: the filter and the match column do not wrap
		const uint32_t full[8] = { 0xffffffffu, 0xffffffffu, 0, 0, 0, 7, 0, 0 };
		if (pileMatches(0xffffffffu, full) != 0 || !pilePasses(0xffffffffu, full, 0xffffffffull, 1.0) || pilePasses(0xffffffffu, full, 0x100000000ull, 0.0)) die("full words");
		const uint32_t half[8] = { 0, 0, 2, 0, 0, 0, 0, 0 };
		if (!pilePasses(4, half, 2, 0.5) || pilePasses(4, half, 3, 0.0) || pilePasses(4, half, 0, 0.5000001) || pilePasses(0, half, 0, 0.0)) die("the filter");
	}
	Graph g;
	Counts c;
	std::ifstream in(argv[1]);
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream f(line);
		std::string kind;
		f >> kind;
		if (kind == "G") {
			size_t n; f >> n;
			g.names.assign(n, ""); g.letters.assign(n, ""); g.segStart.assign(n + 1, 0);
			for (size_t s = 0; s < n; s++) { std::string l, h; f >> l >> h; g.letters[s] = unhex(l); g.names[s] = unhex(h); g.segStart[s + 1] = g.segStart[s] + g.letters[s].size(); }
			c.depth.assign(g.segStart[n], 0); c.rows.assign(8 * g.segStart[n], 0); c.plain.assign(8 * g.segStart[n], 0); c.bad = false;
		} else if (kind == "T") {
			size_t n; std::string h; f >> n >> h;
			const std::string read = unhex(h);
			std::vector<PileLane> cells(n);
			for (auto& cell : cells) f >> cell.node >> cell.offset >> cell.seqPos;
			if (n) addByLanes(g, cells, read, c);
		} else if (kind == "E") {
			uint64_t minAlt, first, count; double minFraction;
			f >> minAlt >> minFraction >> first >> count;
			if (c.bad) { std::cout << "BAD\n"; continue; }
			if (c.rows != c.plain) die("the lanes' rows differ from the plain loop's");
			for (uint64_t i = 0; i < c.depth.size(); i++) {
				uint64_t others = 0;
				for (uint32_t k = 0; k <= PILE_DEL; k++) others += c.rows[i * 8 + k];
				if (others > c.depth[i]) die("more mismatches and deletions than depth");
				if (c.depth[i] == 0 && (c.rows[i * 8 + PILE_INS_AFTER] || c.rows[i * 8 + PILE_INS_BEFORE])) die("an insertion on a base nothing covers");
			}
			std::cout << "P " << hex(pileupTable(g, c, first, count, minAlt, minFraction)) << "\n";
		} else if (kind == "Z") {
			c.depth.assign(c.depth.size(), 0); c.rows.assign(c.rows.size(), 0); c.plain.assign(c.plain.size(), 0); c.bad = false;
		}
	}
	return 0;
}
