// csrc/hip/gc_coverage_core.hpp as an ordinary program (g++, also under -fsanitize=address,undefined): the per-cell rule, the strand flip and the grouping of a chunk's
// covering lanes into runs of one segment over 64 emulated lanes; the run marking of the base table per tile, and the lines of both tables, each written into exactly
// the bytes its length function counted. tests/test_coverage_host.py writes the cases, runs this and holds what it prints to tests/coverage_model.py.
//   G n (length hex(name)) x n      the graph's segments in internal order ("-": no name)
//   T n (node offset) x n           one trace, added to the accumulators
//   E                               -> "S hex(segment table)" and "B hex(base table)", the accumulators back to zero
// bases[] comes from the run-opening lanes and depth[] from the covering lanes, as in the kernel; before a table is printed every bases[s] must equal the sum of the
// segment's depth and the plain loop's count (exit 1 otherwise).
#include "gc_coverage_core.hpp"
#include <cstdio>
#include <cstdlib>
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

struct Graph { std::vector<std::string> names; std::vector<uint64_t> segStart; };
struct Counts { std::vector<uint64_t> bases, plain; std::vector<uint32_t> depth; };

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(1); }

// the kernel's loop with the wave spelled out
static void addByLanes(const Graph& g, const std::vector<CovLane>& cells, Counts& c)
{
	const uint32_t n = (uint32_t)cells.size();
	CovLane carry { 0, 0 };
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t nValid = n - base < 64 ? n - base : 64;
		CovLane lanes[64];
		for (uint32_t l = 0; l < 64; l++) lanes[l] = cells[base + l < n ? base + l : n - 1];   // (lanes past the end load the last cell, as the kernel does)
		uint64_t coverMask = 0, openMask = 0;
		covChunk(lanes, nValid, base, carry, coverMask, openMask);
		if (nValid < 64 && (coverMask >> nValid)) die("a lane past the trace's end covers");
		if (openMask & ~coverMask) die("a lane opens a run and does not cover");
		uint32_t inRuns = 0;
		for (uint32_t l = 0; l < nValid; l++) {
			if (!((coverMask >> l) & 1)) continue;
			const uint32_t seg = covSegment(lanes[l].node);
			const uint64_t length = g.segStart.at(seg + 1) - g.segStart.at(seg);
			if (lanes[l].offset >= length) die("a cell outside its segment");
			c.depth.at(g.segStart[seg] + covForward(lanes[l].node, lanes[l].offset, (uint32_t)length))++;
			if ((openMask >> l) & 1) { const uint32_t run = covRunLength(coverMask, openMask, l); c.bases.at(seg) += run; inRuns += run; }
		}
		if (inRuns != (uint32_t)__builtin_popcountll(coverMask)) die("the runs of a chunk do not add up to its covering lanes");
		carry = lanes[nValid - 1];
	}
	for (uint32_t i = 0; i < n; i++)   // the rule as it is stated
		if (i == 0 || cells[i].node != cells[i - 1].node || cells[i].offset != cells[i - 1].offset) c.plain.at((uint32_t)cells[i].node >> 1)++;
}

static std::string segmentTable(const Graph& g, const Counts& c)
{
	std::string out = "#segment\tlength\tbases\n";
	for (uint64_t s = 0; s + 1 < g.segStart.size(); s++) {
		const uint64_t length = g.segStart[s + 1] - g.segStart[s];
		const std::string& name = g.names[s];
		std::vector<char> line(covSegmentLineLen((uint32_t)name.size(), s, length, c.bases[s]));   // exactly the counted bytes: a longer line is the sanitizer's to find
		if (covSegmentLine(line.data(), name.data(), (uint32_t)name.size(), s, length, c.bases[s]) != line.size()) die("a segment line is not as long as it was counted");
		out.append(line.data(), line.size());
	}
	return out;
}

// the finish step per tile of `tile` bases: starts and ends found by the run rule, the k-th start paired with the k-th end
static std::string baseTable(const Graph& g, const Counts& c, uint64_t tile)
{
	const uint64_t nSeg = g.segStart.size() - 1, nBases = g.segStart[nSeg];
	std::vector<uint64_t> runStart, runEnd;
	for (uint64_t first = 0; first < nBases; first += tile) {
		uint64_t s = covSegmentOfBase(g.segStart.data(), nSeg, first);
		for (uint64_t i = first; i < first + tile && i < nBases; i++) {
			while (i >= g.segStart[s + 1]) s++;
			if (covSegmentOfBase(g.segStart.data(), nSeg, i) != s) die("the segment search and the walk disagree");
			const uint32_t left = i > 0 ? c.depth[i - 1] : 0, here = c.depth[i], right = i + 1 < nBases ? c.depth[i + 1] : 0;
			if (covRunStarts(i == g.segStart[s], left, here)) runStart.push_back(i);
			if (covRunEnds(i + 1 == g.segStart[s + 1], here, right)) runEnd.push_back(i + 1);
		}
	}
	if (runStart.size() != runEnd.size()) die("as many run ends as run starts");
	std::string out;
	for (size_t r = 0; r < runStart.size(); r++) {
		const uint64_t b = runStart[r], e = runEnd[r], s = covSegmentOfBase(g.segStart.data(), nSeg, b), s0 = g.segStart[s];
		if (e <= b || e > g.segStart[s + 1]) die("a run leaves its segment");
		for (uint64_t i = b; i < e; i++) if (c.depth[i] != c.depth[b]) die("a run of unequal depth");
		const std::string& name = g.names[s];
		std::vector<char> line(covRunLineLen((uint32_t)name.size(), s, b - s0, e - s0, c.depth[b]));
		if (covRunLine(line.data(), name.data(), (uint32_t)name.size(), s, b - s0, e - s0, c.depth[b]) != line.size()) die("a run line is not as long as it was counted");
		out.append(line.data(), line.size());
	}
	return out;
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: coverage_host_test cases.txt\n"); return 2; }
	{
		const uint64_t values[] = { 0, 9, 10, 99, 100, 4294967295ull, 4294967296ull, 18446744073709551615ull };
		for (uint64_t v : values) {
			char buf[24];
			const uint32_t n = covDecimal(buf, v);
			if (n != covDecimalLen(v) || std::string(buf, n) != std::to_string(v)) die("decimal formatting");
		}
		if (covSatAdd(0xfffffff0u, 0x20u) != 0xffffffffu || covSatAdd(7u, 8u) != 15u || covSatAdd(0xffffffffu, 0u) != 0xffffffffu) die("saturating add");
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
			g.names.assign(n, ""); g.segStart.assign(n + 1, 0);
			for (size_t s = 0; s < n; s++) { uint64_t length; std::string h; f >> length >> h; g.names[s] = unhex(h); g.segStart[s + 1] = g.segStart[s] + length; }
			c.bases.assign(n, 0); c.plain.assign(n, 0); c.depth.assign(g.segStart[n], 0);
		} else if (kind == "T") {
			size_t n; f >> n;
			std::vector<CovLane> cells(n);
			for (auto& cell : cells) f >> cell.node >> cell.offset;
			if (n) addByLanes(g, cells, c);
		} else if (kind == "E") {
			for (size_t s = 0; s + 1 < g.segStart.size(); s++) {
				uint64_t sum = 0;
				for (uint64_t i = g.segStart[s]; i < g.segStart[s + 1]; i++) sum += c.depth[i];
				if (sum != c.bases[s] || c.plain[s] != c.bases[s]) { fprintf(stderr, "segment %zu: runs %llu, depth %llu, plain loop %llu\n", s, (unsigned long long)c.bases[s], (unsigned long long)sum, (unsigned long long)c.plain[s]); return 1; }
			}
			const std::string table = baseTable(g, c, 2048);
			for (uint64_t tile : { 1ull, 7ull, 64ull }) if (baseTable(g, c, tile) != table) die("the base table depends on the tile size");
			std::cout << "S " << hex(segmentTable(g, c)) << "\nB " << hex(table) << "\n";
			c.bases.assign(c.bases.size(), 0); c.plain.assign(c.plain.size(), 0); c.depth.assign(c.depth.size(), 0);
		}
	}
	return 0;
}
