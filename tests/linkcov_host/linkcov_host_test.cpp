// csrc/hip/gc_coverage_links_core.hpp as an ordinary program (g++, also under -fsanitize=address,undefined): the canonical key, the search over the sorted keys, the
// traversal step over 64 emulated lanes with the carry, and the lines of the link table and of the tagged GFA, each written into exactly the bytes its length function
// counted. tests/test_linkcov_host.py writes the cases, runs this and holds what it prints to tests/link_coverage_model.py.
//   G n (hex(name) letters bases) x n   the graph's segments in internal order ("-": no name)
//   L n (u v) x n                       the graph's links, canonical and ascending
//   K u v                               -> "K cu cv index" (index = n: no link)
//   T n (node offset) x n               one trace, its traversals added to the counters
//   C index count                       sets a counter
//   E                                   -> "T hex(link table)", "S hex(S lines)", "L hex(L lines)", "s hex(supported S lines)", "l hex(supported L lines)"; the counters back to zero
#include "gc_coverage_links_core.hpp"
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
static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(1); }

struct Graph { std::vector<std::string> names, letters; std::vector<uint64_t> bases, keys, counts, plain; };

// the kernel's traversal step with the wave spelled out
static void addByLanes(Graph& g, const std::vector<CovLane>& cells)
{
	const uint32_t n = (uint32_t)cells.size();
	const uint64_t nLinks = g.keys.size();
	CovLane carry { 0, 0 };
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t nValid = n - base < 64 ? n - base : 64;
		CovLane lanes[64];
		for (uint32_t l = 0; l < 64; l++) lanes[l] = cells[base + l < n ? base + l : n - 1];   // (lanes past the end load the last cell, as the kernel does)
		std::vector<uint64_t> key(nValid);   // exactly the valid lanes: a write past them is the sanitizer's to find
		const uint64_t mask = covLinkChunk(lanes, nValid, base, carry, key.data());
		if (nValid < 64 && (mask >> nValid)) die("a lane past the trace's end traverses");
		if (base == 0 && (mask & 1)) die("cell 0 traverses");
		for (uint32_t l = 0; l < nValid; l++) {
			if (!((mask >> l) & 1)) continue;
			const uint64_t link = covLinkFind(g.keys.data(), nLinks, key[l]);
			if (link >= nLinks) die("a traversal along no link");
			g.counts[link]++;
		}
		carry = lanes[nValid - 1];
	}
	for (uint32_t i = 1; i < n; i++)   // the rule as it is stated
		if (cells[i].node != cells[i - 1].node) {
			const uint32_t u = (uint32_t)cells[i - 1].node, v = (uint32_t)cells[i].node;
			const uint64_t own = (uint64_t)u << 32 | v, mate = (uint64_t)(v ^ 1) << 32 | (u ^ 1);
			for (uint64_t k = 0; k < nLinks; k++) if (g.keys[k] == own || g.keys[k] == mate) g.plain[k]++;
		}
}

template <typename LenF, typename WriteF>
static void line(std::string& out, LenF len, WriteF write)
{
	std::vector<char> buf(len());   // exactly the counted bytes
	if (write(buf.data()) != buf.size()) die("a line is not as long as it was counted");
	out.append(buf.data(), buf.size());
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: linkcov_host_test cases.txt\n"); return 2; }
	Graph g;
	std::ifstream in(argv[1]);
	std::string text;
	while (std::getline(in, text)) {
		std::istringstream f(text);
		std::string kind;
		f >> kind;
		if (kind == "G") {
			size_t n; f >> n;
			g.names.assign(n, ""); g.letters.assign(n, ""); g.bases.assign(n, 0);
			for (size_t s = 0; s < n; s++) { std::string h; f >> h >> g.letters[s] >> g.bases[s]; g.names[s] = unhex(h); if (g.letters[s] == "-") g.letters[s].clear(); }
		} else if (kind == "L") {
			size_t n; f >> n;
			g.keys.assign(n, 0);
			for (auto& k : g.keys) { uint32_t u, v; f >> u >> v; k = (uint64_t)u << 32 | v; if (covLinkKey(u, v) != k) die("a link that is not canonical"); }
			for (size_t k = 1; k < n; k++) if (g.keys[k - 1] >= g.keys[k]) die("the links do not ascend");
			g.counts.assign(n, 0); g.plain.assign(n, 0);
			for (size_t k = 0; k < n; k++) {   // every link is found, from either strand; what lies between two links is not
				const uint32_t u = covLinkFrom(g.keys[k]), v = covLinkTo(g.keys[k]);
				if (covLinkFind(g.keys.data(), n, covLinkKey(u, v)) != k || covLinkFind(g.keys.data(), n, covLinkKey(v ^ 1, u ^ 1)) != k) die("a link is not found");
				if (covLinkFind(g.keys.data(), n, g.keys[k] + 1) != (k + 1 < n && g.keys[k + 1] == g.keys[k] + 1 ? k + 1 : n)) die("a key behind a link is found");
			}
			if (covLinkFind(g.keys.data(), 0, 5) != 0) die("a search over no links");
		} else if (kind == "K") {
			uint32_t u, v; f >> u >> v;
			const uint64_t key = covLinkKey(u, v);
			if (key != covLinkKey(v ^ 1, u ^ 1)) die("a pair and its mate differ in their canonical form");
			std::cout << "K " << covLinkFrom(key) << " " << covLinkTo(key) << " " << covLinkFind(g.keys.data(), g.keys.size(), key) << "\n";
		} else if (kind == "T") {
			size_t n; f >> n;
			std::vector<CovLane> cells(n);
			for (auto& cell : cells) f >> cell.node >> cell.offset;
			if (n) addByLanes(g, cells);
		} else if (kind == "C") {
			size_t k; uint64_t c; f >> k >> c;
			g.counts.at(k) = c; g.plain.at(k) = c;
		} else if (kind == "E") {
			if (g.counts != g.plain) die("the lanes and the plain loop count differently");
			std::string table = "#from\tfrom_orient\tto\tto_orient\ttraversals\n", gfaL, gfaS, keptL, keptS;
			for (size_t k = 0; k < g.keys.size(); k++) {
				const uint32_t u = covLinkFrom(g.keys[k]), v = covLinkTo(g.keys[k]);
				const std::string& a = g.names.at(u >> 1); const std::string& b = g.names.at(v >> 1);
				const uint64_t c = g.counts[k];
				line(table, [&] { return covLinkLineLen((uint32_t)a.size(), (uint32_t)b.size(), u, v, c); }, [&](char* out) { return covLinkLine(out, a.data(), (uint32_t)a.size(), b.data(), (uint32_t)b.size(), u, v, c); });
				std::string one;
				line(one, [&] { return covGfaLinkLineLen((uint32_t)a.size(), (uint32_t)b.size(), u, v, c); }, [&](char* out) { return covGfaLinkLine(out, a.data(), (uint32_t)a.size(), b.data(), (uint32_t)b.size(), u, v, c); });
				gfaL += one;
				if (c) keptL += one;
			}
			for (size_t s = 0; s < g.names.size(); s++) {
				const std::string& name = g.names[s]; const std::string& letters = g.letters[s];
				std::string one;
				line(one, [&] { return covGfaSegmentLineLen((uint32_t)name.size(), s, letters.size(), g.bases[s]); },
					[&](char* out) { return covGfaSegmentLine(out, name.data(), (uint32_t)name.size(), s, letters.data(), letters.size(), g.bases[s]); });
				if (covGfaSegmentLettersAt((uint32_t)name.size(), s) + letters.size() > one.size() || one.compare(covGfaSegmentLettersAt((uint32_t)name.size(), s), letters.size(), letters) != 0) die("the letters are not where the kernel would write them");
				gfaS += one;
				if (g.bases[s]) keptS += one;
			}
			std::cout << "T " << hex(table) << "\nS " << hex(gfaS) << "\nL " << hex(gfaL) << "\ns " << hex(keptS) << "\nl " << hex(keptL) << "\n";
			g.counts.assign(g.counts.size(), 0); g.plain.assign(g.plain.size(), 0);
		}
	}
	return 0;
}
