// The node-record accessors of the whole-read kernel (hip/gc_device.hpp: gcNodeRec, recLength, gcNodeLength, recNodeSeq, recRank, recOutRange, recInRange,
// gcOutAdj, gcInAdj) compiled for the host and held to the graph arrays they replace, for every node of random CSR graphs. The records are made with the
// formula of k_build_node_rec (hip/gc_extend_frag.hip). Every array has exactly the size the device gives it, so a read behind an end (record n, outOff[n + 1],
// a plain node's ambSeq words) is an error under -fsanitize=address. Test infrastructure.
#define __HIP_PLATFORM_AMD__ 1
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __clzll(long long x) { return __builtin_clzll(x); }
#include "../../graphchainer_amd/csrc/hip/gc_device.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace gcdev;

struct Graph {
	std::vector<uint8_t> nodeLength;
	std::vector<uint64_t> nodeSeq, ambSeq;
	std::vector<uint32_t> inOff, inAdj, outOff, outAdj, componentNumber;
	std::vector<NodeRec> rec;
	DGraph d {};
};

static const uint32_t SPECIAL_DEGREES[] = { 0, 1, 254, 255, 256, 300 };

// one CSR with the special degrees at random nodes and at node n - 1 (in turn, by `lastKind`); the in- and the out-CSR are drawn independently: the accessors
// do not relate them
static void randomCsr(std::mt19937_64& rng, uint32_t n, uint32_t lastKind, std::vector<uint32_t>& off, std::vector<uint32_t>& adj)
{
	std::vector<uint32_t> deg(n);
	for (uint32_t v = 0; v < n; v++) deg[v] = (uint32_t)(rng() % 4);
	for (uint32_t k = 0; k < 6; k++) for (int rep = 0; rep < 3; rep++) deg[rng() % n] = SPECIAL_DEGREES[k];
	deg[n - 1] = SPECIAL_DEGREES[lastKind % 6];
	deg[0] = SPECIAL_DEGREES[(lastKind + 3) % 6];
	off.assign(n + 1, 0);
	for (uint32_t v = 0; v < n; v++) off[v + 1] = off[v] + deg[v];
	adj.resize(off[n]);
	for (auto& t : adj) t = (uint32_t)(rng() % n);
}

static Graph randomGraph(uint64_t seed, uint32_t n, uint32_t nAmbiguous, uint32_t lastKind)
{
	std::mt19937_64 rng(seed);
	Graph g;
	const uint32_t firstAmbiguous = n - nAmbiguous;
	g.nodeLength.resize(n); g.componentNumber.resize(n);
	for (uint32_t v = 0; v < n; v++) { g.nodeLength[v] = (uint8_t)(1 + rng() % 64); g.componentNumber[v] = (uint32_t)rng(); }
	for (int rep = 0; rep < 4; rep++) { g.nodeLength[rng() % n] = 1; g.nodeLength[rng() % n] = 64; }
	g.nodeLength[n - 1] = lastKind % 2 ? 64 : 1;
	g.nodeLength[0] = lastKind % 2 ? 1 : 64;
	g.nodeSeq.resize(2 * (size_t)firstAmbiguous); g.ambSeq.resize(4 * (size_t)nAmbiguous);
	for (auto& w : g.nodeSeq) w = rng();
	for (auto& w : g.ambSeq) w = rng();
	randomCsr(rng, n, lastKind, g.outOff, g.outAdj);
	randomCsr(rng, n, lastKind + 1, g.inOff, g.inAdj);
	g.rec.resize(n);
	for (uint32_t v = 0; v < n; v++) {   // k_build_node_rec
		NodeRec& r = g.rec[v];
		const uint32_t outBegin = g.outOff[v], inBegin = g.inOff[v];
		const uint32_t outDeg = g.outOff[v + 1] - outBegin, inDeg = g.inOff[v + 1] - inBegin;
		const bool plain = v < firstAmbiguous;
		r.comp = g.componentNumber[v]; r.outOff = outBegin; r.inOff = inBegin;
		r.meta = (uint32_t)g.nodeLength[v] | (plain ? 0u : NODEREC_SLOW) | ((outDeg < 255u ? outDeg : 255u) << 8) | ((inDeg < 255u ? inDeg : 255u) << 16);
		r.w0 = plain ? g.nodeSeq[2 * (size_t)v] : 0ull;
		r.w1 = plain ? g.nodeSeq[2 * (size_t)v + 1] : 0ull;
	}
	g.d.nNodes = n; g.d.firstAmbiguous = firstAmbiguous;
	g.d.nodeLength = g.nodeLength.data(); g.d.nodeSeq = g.nodeSeq.data(); g.d.ambSeq = g.ambSeq.data();
	g.d.inOff = g.inOff.data(); g.d.inAdj = g.inAdj.data(); g.d.outOff = g.outOff.data(); g.d.outAdj = g.outAdj.data();
	g.d.componentNumber = g.componentNumber.data();
	g.d.nodeRec = g.rec.data();
	return g;
}

static unsigned long long g_checks = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { fprintf(stderr, "graph %llu node %u: %s (line %d)\n", (unsigned long long)seed, v, #cond, __LINE__); exit(1); } } while (0)

int main()
{
	unsigned long long nodes = 0, seen[6][2] = {}, ambiguousNodes = 0, length1 = 0, length64 = 0;
	for (uint64_t seed = 1; seed <= 12; seed++) {
		const uint32_t n = 2000 + (uint32_t)(seed * 331 % 1500);
		const uint32_t nAmbiguous = seed % 4 == 0 ? 0 : seed % 4 == 1 ? 1 : 37 + (uint32_t)seed;   // (none: the last node is a plain one; one: it is the only ambiguous one)
		const Graph G = randomGraph(seed, n, nAmbiguous, (uint32_t)seed);
		const DGraph& g = G.d;
		for (uint32_t v = 0; v < n; v++) {
			const NodeRec r = gcNodeRec(g, v);
			CHECK(recLength(r) == g.nodeLength[v]);
			CHECK(gcNodeLength(g, v) == g.nodeLength[v]);
			CHECK(recRank(r) == g.componentNumber[v]);
			const NodeSeq want = loadNodeSeq(g, v), got = recNodeSeq(g, v, r);
			CHECK(got.ambiguous == want.ambiguous && got.w0 == want.w0 && got.w1 == want.w1 && got.w2 == want.w2 && got.w3 == want.w3);
			const EdgeRange outs = recOutRange(g, v, r), ins = recInRange(g, v, r);
			CHECK(outs.begin == g.outOff[v] && outs.end == g.outOff[v + 1]);
			CHECK(ins.begin == g.inOff[v] && ins.end == g.inOff[v + 1]);
			for (uint32_t e = outs.begin; e < outs.end; e++) CHECK(gcOutAdj(g, e) == g.outAdj[e]);
			for (uint32_t e = ins.begin; e < ins.end; e++) CHECK(gcInAdj(g, e) == g.inAdj[e]);
			for (int k = 0; k < 6; k++) { seen[k][0] += outs.end - outs.begin == SPECIAL_DEGREES[k]; seen[k][1] += ins.end - ins.begin == SPECIAL_DEGREES[k]; }
			ambiguousNodes += want.ambiguous; length1 += g.nodeLength[v] == 1; length64 += g.nodeLength[v] == 64;
		}
		nodes += n;
	}
	for (int k = 0; k < 6; k++) if (!seen[k][0] || !seen[k][1]) { fprintf(stderr, "no node of degree %u\n", SPECIAL_DEGREES[k]); return 1; }
	if (!ambiguousNodes || !length1 || !length64) { fprintf(stderr, "a kind of node is missing\n"); return 1; }
	printf("NODE_REC_HOST_OK graphs 12 nodes %llu checks %llu ambiguous %llu length1 %llu length64 %llu\n", nodes, g_checks, ambiguousNodes, length1, length64);
	return 0;
}
