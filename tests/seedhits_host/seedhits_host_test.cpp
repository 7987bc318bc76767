// The per-hit parts of the caller-supplied seed path (csrc/hip/gc_seedhits_core.hpp), compiled for the host:
//   resolve  seedHitResolve against AlignmentGraph::GetUnitigNode + the split node's nodeOffset (what orderSeedsByChaining does per hit, src/GraphAligner.h:250-252) on every
//            (bigraph id, offset) of a graph, and its refusals: an id beyond the graph, an offset at and beyond the original node's size, a read position at and beyond the read's length
//   windows  the prefix-maximum rule of seedWindow against the literal two-pointer loop of src/Aligner.cpp:672-679 on random seed lists with matchLen 2..100, duplicates and up
//            to 200 seeds; the running maximum is made the way the kernel makes it - 64 lanes a turn, Hillis-Steele steps of seedMaxScanStep, a carry between turns
// usage: seedhits_host_test graph.gfa [short]   (short: the graph must have a segment whose last split node is shorter than 64 - the case is then known to be covered)
#include "gc_graph.hpp"
#include "gc_seedhits_core.hpp"
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace gcdev;

static std::vector<uint32_t> runningMaxByTurns(const std::vector<uint32_t>& ends)
{
	std::vector<uint32_t> out(ends.size());
	uint32_t carry = 0;
	for (size_t base = 0; base < ends.size(); base += 64) {
		uint32_t v[64], before[64];
		for (uint32_t lane = 0; lane < 64; lane++) v[lane] = base + lane < ends.size() ? ends[base + lane] : 0;
		for (uint32_t d = 1; d < 64; d <<= 1) {
			std::copy(v, v + 64, before);
			for (uint32_t lane = 0; lane < 64; lane++) v[lane] = seedMaxScanStep(before[lane], lane >= d ? before[lane - d] : before[lane], lane, d);   // (a lane below d reads itself, as __shfl_up gives it)
		}
		for (uint32_t lane = 0; lane < 64; lane++) { v[lane] = std::max(v[lane], carry); if (base + lane < ends.size()) out[base + lane] = v[lane]; }
		carry = v[63];
	}
	return out;
}

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	gc::GfaGraph gfa = gc::GfaGraph::LoadFromFile(argv[1]);
	gc::AlignmentGraph graph = gc::AlignmentGraph::BuildFromGFA(gfa);
	// the flat tables as the device holds them (uploadGraph)
	int maxId = -1;
	for (size_t i = 0; i < graph.NodeSize(); i++) maxId = std::max(maxId, graph.nodeIDs[i]);
	const size_t nB = (size_t)maxId + 1;
	std::vector<uint32_t> origSize(nB, 0), lookupOff(nB + 1, 0), lookup, nodeOffset(graph.NodeSize());
	for (size_t i = 0; i < graph.NodeSize(); i++) nodeOffset[i] = (uint32_t)graph.nodeOffset[i];
	for (size_t id = 0; id < nB; id++) {
		const bool known = graph.nodeLookup.contains((int)id);
		lookupOff[id + 1] = lookupOff[id] + (known ? (uint32_t)graph.nodeLookup.at((int)id).size() : 0u);
		if (known) { origSize[id] = (uint32_t)graph.originalNodeSize.at((int)id); for (size_t s : graph.nodeLookup.at((int)id)) lookup.push_back((uint32_t)s); }
	}
	const SeedLookup view { origSize.data(), lookupOff.data(), lookup.data(), nodeOffset.data(), (uint32_t)nB };
	size_t resolved = 0, refused = 0, lastShort = 0;
	for (size_t id = 0; id < nB; id++) {
		if (!origSize[id]) continue;
		for (uint32_t o = 0; o < origSize[id]; o++, resolved++) {
			const SeedHit h { (int32_t)(id / 2), o, 5, 15, 0, (uint32_t)(id & 1) };
			uint32_t node = ~0u, off = ~0u;
			if (seedHitResolve(view, h, 6, node, off) != SEED_HIT_OK) { printf("MISMATCH refused %zu %u\n", id, o); return 1; }
			const size_t want = graph.GetUnitigNode((int)id, o);
			if (node != want || off != o - graph.nodeOffset[want] || off >= graph.nodeLength[want]) { printf("MISMATCH resolve %zu %u: %u %u, GetUnitigNode %zu\n", id, o, node, off, want); return 1; }
			if (o + 1 == origSize[id] && graph.nodeLength[want] < 64 && lookupOff[id + 1] - lookupOff[id] > 1) lastShort++;
		}
		uint32_t node = 7, off = 7;
		const SeedHit atEnd { (int32_t)(id / 2), origSize[id], 0, 15, 0, (uint32_t)(id & 1) }, beyond { (int32_t)(id / 2), 0xffffffffu, 0, 15, 0, (uint32_t)(id & 1) };
		const SeedHit posAtEnd { (int32_t)(id / 2), 0, 6, 15, 0, (uint32_t)(id & 1) }, strand { (int32_t)(id / 2), 0, 0, 15, 0, 2 };
		if (seedHitResolve(view, atEnd, 6, node, off) != SEED_HIT_OFFSET || seedHitResolve(view, beyond, 6, node, off) != SEED_HIT_OFFSET || seedHitResolve(view, posAtEnd, 6, node, off) != SEED_HIT_SEQPOS
			|| seedHitResolve(view, strand, 6, node, off) != SEED_HIT_NO_NODE || node != 7 || off != 7) { printf("MISMATCH refusal %zu\n", id); return 1; }
		refused += 4;
	}
	{
		uint32_t node = 7, off = 7;
		const SeedHit negative { -1, 0, 0, 15, 0, 0 }, past { (int32_t)(nB / 2 + 1), 0, 0, 15, 0, 0 }, huge { 0x7fffffff, 0, 0, 15, 0, 1 };
		if (seedHitResolve(view, negative, 6, node, off) != SEED_HIT_NO_NODE || seedHitResolve(view, past, 6, node, off) != SEED_HIT_NO_NODE || seedHitResolve(view, huge, 6, node, off) != SEED_HIT_NO_NODE) { printf("MISMATCH id refusal\n"); return 1; }
	}
	// ---- windows
	std::mt19937_64 rng(11);
	size_t windows = 0, lists = 0, turns = 0, shrunk = 0;
	for (int round = 0; round < 4000; round++) {
		const uint32_t len = 40 + (uint32_t)(rng() % 1500), splitLen = 16 + (uint32_t)(rng() % 49), splitGap = 1 + (uint32_t)(rng() % 70);
		const uint32_t nS = (uint32_t)(rng() % 201);
		std::vector<std::pair<uint32_t, uint32_t>> seeds(nS);   // (seqPos, matchLen), sorted by seqPos (the order among equal positions is the unstable sort's: any)
		for (auto& s : seeds) { s.first = (uint32_t)(rng() % len); s.second = 2 + (uint32_t)(rng() % 99); }
		for (uint32_t i = 0; i + 1 < nS; i += 7) seeds[i + 1] = seeds[i];   // duplicates
		if (nS > 3 && round % 3 == 0) for (uint32_t i = 0; i + 2 < nS; i += 5) seeds[i + 2].first = seeds[i].first;   // one position, several matchLen
		std::stable_sort(seeds.begin(), seeds.end(), [](const auto& l, const auto& r) { return l.first < r.first; });
		std::vector<uint32_t> ends(nS);
		for (uint32_t i = 0; i < nS; i++) ends[i] = seeds[i].first + seeds[i].second;
		const std::vector<uint32_t> endMax = runningMaxByTurns(ends);
		for (uint32_t i = 0; i < nS; i++) if (endMax[i] != *std::max_element(ends.begin(), ends.begin() + i + 1)) { printf("MISMATCH running maximum %d %u\n", round, i); return 1; }
		size_t sl = 0, sr = 0;
		for (size_t l = 0; l + splitLen <= len; l += splitGap, windows++) {
			while (sr < nS && (size_t)seeds[sr].first + seeds[sr].second <= l + splitLen) sr++;
			while (sl < sr && seeds[sl].first < l) sl++;
			uint32_t gl = ~0u, gr = ~0u;
			seedWindow([&](uint32_t i) { return endMax[i]; }, [&](uint32_t i) { return seeds[i].first; }, nS, l, splitLen, gl, gr);
			if (gl != sl || gr != sr) { printf("MISMATCH window %d l=%zu: [%u, %u), two pointers [%zu, %u)\n", round, l, gl, gr, sl, (unsigned)sr); return 1; }
			// (where the rule differs from a search on the seeds' own ends: a later seed that ends earlier than one before it)
			if (sr < nS && std::any_of(ends.begin() + sr, ends.end(), [&](uint32_t e) { return e <= l + splitLen; })) shrunk++;
		}
		lists++; turns += (nS + 63) / 64;
	}
	const bool needShort = argc > 2 && std::string(argv[2]) == "short";
	if (turns < 2 * lists || shrunk < 1000 || (needShort && lastShort < 1)) { printf("WEAK turns %zu lists %zu shrunk %zu lastShort %zu\n", turns, lists, shrunk, lastShort); return 1; }
	printf("OK %zu resolved, %zu refused, %zu windows of %zu lists (%zu where the seeds' own ends are not sorted)\n", resolved, refused, windows, lists, shrunk);
	return 0;
}
