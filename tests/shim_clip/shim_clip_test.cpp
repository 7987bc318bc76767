// Drives include/graphchainer_amd_shim.hpp with precise clipping and the X-drop: gcshim::bind() with a gc_params_ext { precise_clipping = CUTOFF, x_drop = XDROP }, then
// AlignOneWay (whole read, src/Aligner.cpp:565) with the matching preciseClipping / preciseClippingIdentityCutoff / Xdropcutoff (accepted: the replay of the bound batch)
// and with differing ones (refused: std::invalid_argument). An X-drop bound without a cut-off runs with 0.66 (src/AlignerMain.cpp:443-448), and that is what a call gives.
// Minimal definitions of the reference's types as in tests/shim/shim_test.cpp.
//   shim_clip_test graph.gfa CUTOFF XDROP READ [READ ...]      (CUTOFF 0: off; XDROP 0: off)
// Prints, per read: ALN <read> <start> <end> <score> <trace cells> for every whole-read alignment, then REFUSED <read> <n> <of> for the calls with differing values.
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

static AlignmentResult alignWhole(const std::string& sequence, const std::vector<SeedHit>& seeds, bool preciseClipping, double cutoff, int xDrop)
{
	AlignmentGraph alignmentGraph;
	GraphAlignerCommon<size_t, int32_t, uint64_t>::AlignerGraphsizedState reusableState;
	return AlignOneWay(alignmentGraph, "r", sequence, 10, 0, std::numeric_limits<size_t>::max(), true, true, seeds, reusableState, true, false, preciseClipping, 1, -1, false, cutoff, xDrop, -1, -1, 0);
}

int main(int argc, char** argv)
{
	if (argc < 5) { fprintf(stderr, "usage: shim_clip_test graph.gfa CUTOFF XDROP READ...\n"); return 2; }
	gc_graph* graph = nullptr;
	gc_seeder* seeder = nullptr;
	int rc = gc_graph_create_from_gfa(argv[1], &graph);
	if (rc == GC_ERR_DEVICE) { printf("NO_DEVICE\n"); return 0; }
	if (rc != GC_OK || gc_seeder_create(graph, 15, 20, 1.0 - 0.001, &seeder) != GC_OK) { fprintf(stderr, "%s\n", gc_last_error()); return 1; }
	const double cutoff = atof(argv[2]);
	const int xDrop = atoi(argv[3]);
	gc_params gp;
	gc_params_default(&gp);
	gc_params_ext ext;
	gc_params_ext_default(&ext);
	ext.precise_clipping = cutoff;
	ext.x_drop = xDrop;
	gcshim::bind(graph, seeder, gp, &ext);
	// what the reference's front end hands AlignOneWay for these options (src/AlignerMain.cpp:300-322,443-448)
	const double runCutoff = cutoff != 0 ? cutoff : (xDrop > 0 ? 0.66 : 0.0);
	const bool clipping = runCutoff != 0;
	for (int a = 4; a < argc; a++) {
		const std::string sequence = argv[a];
		std::vector<SeedHit> seeds = gcshim::getSeeds(sequence, 10);
		gcshim::currentRead() = sequence;
		AlignmentResult whole;
		try { whole = alignWhole(sequence, seeds, clipping, clipping ? runCutoff : 0.5, xDrop); }   // (with clipping off the cut-off is not read: 0.5 is the reference's unused default)
		catch (const std::exception& e) { fprintf(stderr, "the shim refused the bound values: %s\n", e.what()); return 1; }
		for (const auto& item : whole.alignments)
			printf("ALN %d %zu %zu %zu %zu\n", a - 4, item.alignmentStart, item.alignmentEnd, item.alignmentScore, item.trace->trace.size());
		int refused = 0, tried = 0;
		auto differing = [&](bool pc, double c, int x) { tried++; try { alignWhole(sequence, seeds, pc, c, x); } catch (const std::invalid_argument&) { refused++; } };
		differing(!clipping, clipping ? 0.5 : 0.66, xDrop);              // clipping switched
		if (clipping) differing(true, runCutoff + 0.01, xDrop);        // another cut-off
		differing(clipping, clipping ? runCutoff : 0.5, xDrop + 1);     // another X-drop
		printf("REFUSED %d %d %d\n", a - 4, refused, tried);
	}
	gc_seeder_destroy(seeder);
	gc_graph_destroy(graph);
	return 0;
}
