// Drives include/graphchainer_amd_shim.hpp with the seed-extension heuristics: gcshim::bind() with gc_params::seed_extend_density = DENSITY and extra_heuristic = FLAG
// (a density other than -1 binds colinear_chaining = 0, as the library demands), then AlignOneWay (whole read, src/Aligner.cpp:565) with the bound values (accepted: the
// replay of the bound batch), with another density and with the other flag (refused: std::invalid_argument), and the fragment call (src/Aligner.cpp:691) with a density
// of -1 (accepted) and with 0.002 (refused). Minimal definitions of the reference's types as in tests/shim/shim_test.cpp.
//   shim_graphaligner_test graph.gfa DENSITY FLAG READ [READ ...]
// Prints, per read: ALN <read> <start> <end> <score> <trace cells> for every whole-read alignment, EXTENDED <read> <seeds extended>, then
// REFUSED <read> <other density> <other flag> <fragment with a density> <fragment with the other flag> ACCEPTED <fragment with -1>.
// Without a GPU the library refuses to create the graph (no CPU fallback): prints NO_DEVICE and exits 0.
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

template <typename LengthType, typename ScoreType, typename Word>
struct GraphAlignerCommon {
	struct MatrixPosition { size_t node = 0, nodeOffset = 0, seqPos = 0; };
	struct TraceItem { MatrixPosition DPposition; bool nodeSwitch = false; char sequenceCharacter = '-', graphCharacter = '-'; };
	struct OnewayTrace { std::vector<TraceItem> trace; ScoreType score = 0; };
	struct AlignerGraphsizedState {};
};
namespace vg { struct Alignment { std::string bytes; bool ParseFromString(const std::string& s) { bytes = s; return true; } }; }
struct SeedHit {
	SeedHit(int nodeID, size_t nodeOffset, size_t seqPos, size_t matchLen, size_t rawSeedGoodness, bool reverse) : nodeID(nodeID), nodeOffset(nodeOffset), seqPos(seqPos), matchLen(matchLen), reverse(reverse),
		alignmentGraphNodeId(std::numeric_limits<size_t>::max()), alignmentGraphNodeOffset(std::numeric_limits<size_t>::max()), rawSeedGoodness(rawSeedGoodness), seedGoodness(0), seedClusterSize(0) {}
	int nodeID; size_t nodeOffset, seqPos, matchLen; bool reverse; size_t alignmentGraphNodeId, alignmentGraphNodeOffset, rawSeedGoodness, seedGoodness, seedClusterSize;
};
struct AlignmentResult {
	struct AlignmentItem {
		AlignmentItem() {}
		AlignmentItem(GraphAlignerCommon<size_t, int32_t, uint64_t>::OnewayTrace&& t, size_t cells, size_t ms) : cellsProcessed(cells), elapsedMilliseconds(ms)
		{ trace = std::make_shared<GraphAlignerCommon<size_t, int32_t, uint64_t>::OnewayTrace>(); *trace = std::move(t); }
		bool alignmentFailed() const { return alignmentEnd == alignmentStart; }
		std::shared_ptr<GraphAlignerCommon<size_t, int32_t, uint64_t>::OnewayTrace> trace;
		std::shared_ptr<vg::Alignment> alignment;   // (the reference's is the protobuf message; here: a holder of its bytes)
		std::string GAFline, corrected;
		size_t seedGoodness = 0, cellsProcessed = 0, elapsedMilliseconds = 0, alignmentStart = 0, alignmentEnd = 0, alignmentScore = std::numeric_limits<size_t>::max();
	};
	std::vector<AlignmentItem> alignments;
	size_t seedsExtended = 0;
};
struct AlignmentGraph { struct Anchor { std::vector<size_t> path; size_t x, y; }; };

#define GC_SHIM_DEFINE_GLOBALS
#include "graphchainer_amd_shim.hpp"

static AlignmentResult align(const std::string& sequence, const std::vector<SeedHit>& seeds, double density, bool flag, long long l, long long r)
{
	AlignmentGraph alignmentGraph;
	GraphAlignerCommon<size_t, int32_t, uint64_t>::AlignerGraphsizedState reusableState;
	return AlignOneWay(alignmentGraph, "r", l < 0 ? sequence : sequence.substr(0, 35), 10, 0, std::numeric_limits<size_t>::max(), true, l < 0, seeds, reusableState, true, false, false, 1, density, flag, 0.5, 0, l, r, 0);
}

static int refused(const std::string& sequence, const std::vector<SeedHit>& seeds, double density, bool flag, long long l, long long r)
{
	try { align(sequence, seeds, density, flag, l, r); } catch (const std::invalid_argument&) { return 1; }
	return 0;
}

int main(int argc, char** argv)
{
	if (argc < 5) { fprintf(stderr, "usage: shim_graphaligner_test graph.gfa DENSITY FLAG READ...\n"); return 2; }
	gc_graph* graph = nullptr;
	gc_seeder* seeder = nullptr;
	int rc = gc_graph_create_from_gfa(argv[1], &graph);
	if (rc == GC_ERR_DEVICE) { printf("NO_DEVICE\n"); return 0; }
	if (rc != GC_OK || gc_seeder_create(graph, 15, 20, 1.0 - 0.001, &seeder) != GC_OK) { fprintf(stderr, "%s\n", gc_last_error()); return 1; }
	const double density = atof(argv[2]);
	const bool flag = atoi(argv[3]) != 0;
	gc_params gp;
	gc_params_default(&gp);
	gp.seed_extend_density = density;
	gp.extra_heuristic = flag ? 1 : 0;
	gp.colinear_chaining = density == -1 ? 1 : 0;
	gcshim::bind(graph, seeder, gp);
	for (int a = 4; a < argc; a++) {
		const std::string sequence = argv[a];
		std::vector<SeedHit> seeds = gcshim::getSeeds(sequence, 10);
		gcshim::currentRead() = sequence;
		AlignmentResult whole;
		try { whole = align(sequence, seeds, density, flag, -1, -1); }
		catch (const std::exception& e) { fprintf(stderr, "the shim refused the bound values: %s\n", e.what()); return 1; }
		for (const auto& item : whole.alignments)
			printf("ALN %d %zu %zu %zu %zu\n", a - 4, item.alignmentStart, item.alignmentEnd, item.alignmentScore, item.trace->trace.size());
		printf("EXTENDED %d %zu\n", a - 4, whole.seedsExtended);
		const double other = density == -1 ? 0.002 : -1;
		printf("REFUSED %d %d %d %d %d ACCEPTED %d\n", a - 4, refused(sequence, seeds, other, flag, -1, -1), refused(sequence, seeds, density, !flag, -1, -1),
			refused(sequence, seeds, 0.002, flag, 0, 1), refused(sequence, seeds, -1, !flag, 0, 1), 1 - refused(sequence, seeds, -1, flag, 0, 1));
	}
	gc_seeder_destroy(seeder);
	gc_graph_destroy(graph);
	return 0;
}
