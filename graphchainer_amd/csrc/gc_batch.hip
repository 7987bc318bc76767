// gc_align_batch: the batch pipeline (BatchRun) - seeding, the whole-read pass on its own thread (WholeReadPass, batch/gc_long_pass.hpp), the fragment pipeline, chaining, stitching,
// edit distances, the decision, output encoding (OutputEncoder, batch/gc_output_encoder.hpp: started on the pass's thread, finished here), result assembly.
#include "gc_runtime.hpp"
#include "batch/gc_long_pass.hpp"
#include "batch/gc_output_encoder.hpp"

extern "C" {

struct BatchRun {
	// ---- the call
	const gc::Switches sw;   // the GC_* switches as they were when the call began (host/gc_switches.hpp)
	const gc_graph* const G; const gc_seeder* const S; const gc_seeds* const H; gc_stream* const st; const gc_reads* const R; const gc_params* const P; const ClipOptions clip; gc_result* const res;   // S: the minimizer index (gc_align_batch), or null and H: the caller's own hits (gc_align_batch_seeded)
	const double tCall, cpuCall;
	double cpuJoined;
	const uint64_t n;                        // reads in the batch
	const gc::AlignmentGraph& hg;
	WorkerPool& pool;
	std::vector<ReadGlue>& glue;             // per-read host records, storage reused across batches
	const hipStream_t stream;                // the fragment pipeline's stream (the whole-read pass has its own: st->longPass)
	int evIdx = 0;
	double tTotal = 0;
	// ---- what the stages hand on (set by the stage named in the comment of each group)
	// seeds()
	double tGlue = 0;
	uint64_t nSlots = 0, nFrags = 0, nSeedsTotal = 0, traceBudget = 0;
	uint32_t maxSlotsPerRead = 1, maxWindowSeeds = 0;
	Fragment* dFrags = nullptr; uint32_t* dFragFirstSeed = nullptr; FragSeed* dReadSeeds = nullptr; ReadChainJob* dJobs = nullptr;   // written by the glue kernels
	LongSeed* dPassSeeds = nullptr;                                          // the same seeds in the whole-read pass's order (long_pass)
	Fragment* frags = nullptr; ReadChainJob* jobs = nullptr;                 // host copies of dFrags / dJobs
	FragSeed* readSeeds = nullptr; uint32_t* fragFirstSeed = nullptr;        // host copies of dReadSeeds / dFragFirstSeed, only with keep_seeds / keep_traces
	hipEvent_t glueCopied = nullptr;   // the host copies of frags / seeds have arrived (waited for before the result assembly)
	double tOrdered = 0;
	unsigned long long* hSmall = nullptr;
	unsigned long long* dCursors = nullptr;
	unsigned long long* dCounters = nullptr;
	const gc::EValueModel evalueModel { clip.on() ? clip.cutoff : 0.7 };   // src/Aligner.cpp:474-482: the clipping cut-off is the model's identity
	// the device output encoder (batch/gc_output_encoder.hpp). The pass's thread runs its first stage through the selectionKnown hook, so it is declared BEFORE the pass:
	// ~WholeReadPass joins a thread that is still running, and members go in reverse order - the hook's target outlives the thread
	OutputEncoder output { sw, G, R, P, st, pool, pass };
	// the whole-read pass: on its own host thread between pass.start() and pass.join(); what the two threads may touch meanwhile is written down in batch/gc_long_pass.hpp
	WholeReadPass pass { sw, G, R, P, clip, st, pool, res, tCall };
	// fragmentPipeline()
	double tDev = 0;
	uint32_t nWork = 0;
	ExtResult* dResults = nullptr;
	PoolCell* dTrace = nullptr;
	AnchorRec* dAnchors = nullptr;
	uint32_t* dFragStatus = nullptr;
	uint32_t* dFragExtended = nullptr;
	uint64_t traceWorst = 0, pathWorst = 0;   // the pools' worst-case sizes (every slot's extensions at full length, 24 path words per slot)
	bool poolsSized = false;
	uint32_t nExtendPairs = 0, nAnchorPairs = 0;   // event pairs recorded around the rounds' k_extend / k_build_anchors launches
	uint32_t poolReruns = 0;
	uint32_t* dReadTies = nullptr;     // per read: fragment extensions whose flattenLastSliceEnd minimum was tied between nodes (k_build_anchors adds them up; gc_result::flatten_ties)
	uint64_t pathCapacity = 0;
	uint32_t* dPathPool = nullptr;
	uint32_t* dChainOut = nullptr;
	uint32_t* dChainLen = nullptr;
	unsigned long long* dChainScore = nullptr;
	uint32_t* dChainStatus = nullptr;
	bool deviceStitch = false;
	StitchInfo* stitchInfo = nullptr;
	uint32_t* hStitchNodes = nullptr;
	uint32_t* dStitchNodes = nullptr;
	uint64_t stitchDenseCap = 0;
	unsigned long long* hStitchCursor = nullptr;
	// resultsBack()
	AnchorRec* anchors = nullptr;
	uint32_t* fragStatus = nullptr;
	uint32_t* fragExtended = nullptr;
	uint32_t* readTies = nullptr;
	uint32_t* chainOut = nullptr;
	uint32_t* chainLen = nullptr;
	unsigned long long* chainScore = nullptr;
	uint32_t* chainStatus = nullptr;
	uint32_t* pathPool = nullptr;
	// r5: the result's dense anchor arrays are made on the device (gc_results.hip) unless the anchors' traces are asked for (keep_traces == 1: the host walks the slots for them anyway)
	bool deviceAnchors = false;
	uint4* hAnchorPerRead = nullptr;                  // (anchors kept, path words, seeds extended, flags) per read
	unsigned long long* hAnchorOff = nullptr;         // [2 r] anchors, [2 r + 1] path words before read r; totals at [2 n], [2 n + 1]
	uint8_t* hAnchorDense = nullptr;                  // the dense arrays as they came down: nine 4-byte arrays, the 8-byte path offsets, the path words
	uint64_t denseAnchors = 0, densePathWords = 0;
	std::vector<ExtResult> extResults;
	std::vector<PoolCell> tracePool;
	bool anchorTraces = false;
	bool stitchNodesPending = false;
	// stitchAndChainDistances()
	const PathSeqJob* chainLetterJobs = nullptr;   // per read: where its stitched path's letters are in dChainLetters
	const char* dChainLetters = nullptr;
	const uint32_t* dChainAltNodes = nullptr;      // the node paths stitched on the host, uploaded for k_chain_pathseq (PathSeqJob::srcOff bit 63)
	const FastChainJob* fastChainJobs = nullptr;   // gc_params::fast_mode, per read: its stitched piece and the chain's (x, y); cells == 0: none
	// withoutChaining()
	std::vector<uint32_t> zeroWords; std::vector<unsigned long long> zeroLongs; std::vector<uint4> zeroPerRead;
	// pass.join()
	double tJoined = 0;

	BatchRun(const gc::Switches& sw, const gc_graph* G, const gc_seeder* S, const gc_seeds* H, gc_stream* st, const gc_reads* R, const gc_params* P, const ClipOptions& clip, gc_result* res, double tCall, double cpuCall)
		: sw(sw), G(G), S(S), H(H), st(st), R(R), P(P), clip(clip), res(res), tCall(tCall), cpuCall(cpuCall), cpuJoined(cpuCall), n(R->offsets.size() - 1), hg(G->host), pool(WorkerPool::batch()), glue(st->glue),
		  stream(st->stream) {}
	BatchRun(const BatchRun&) = delete;
	BatchRun& operator=(const BatchRun&) = delete;

	void mark() { HIP_CHECK(hipEventRecord(st->ev[evIdx++], stream)); }
	double elapsedUs(int a, int b) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, st->ev[a], st->ev[b])); return (double)ms * 1000.0; }

	void run()
	{
		res->n_reads = n;
		tTotal = nowUs();
		// GC_DEBUG_TIMES: CPU time of THIS thread per stage (the waits poll: what a stage costs the host is not its wall time)
		const bool cpuStages = sw.debugTimes;
		double cpuAt = cpuStages ? threadCpuMs() : 0, cpuStage[10] = {}, poolStage[10] = {};
		uint64_t poolAt = pool.cpuUs.load();
		const double processAt = processCpuMs();
		auto stageDone = [&](int k) {
			if (!cpuStages) return;
			const double now = threadCpuMs(); const uint64_t poolNow = pool.cpuUs.load();
			cpuStage[k] += now - cpuAt; poolStage[k] += (poolNow - poolAt) / 1e3;
			cpuAt = now; poolAt = poolNow;
		};
		seeds(); stageDone(0);
		pass.prepare(dPassSeeds, nSeedsTotal); stageDone(1);
		pass.start([this] { output.encodeSelected(); }); stageDone(2);
		if (!P->colinear_chaining) { withoutChaining(); pass.join(tJoined, cpuJoined); stageDone(6); output.choose(stream); stageDone(8); assemble(); stageDone(9); st->batchesDone++; return; }
		fragmentPipeline(); stageDone(3);
		resultsBack(); stageDone(4);
		// r5: the trace pool and the anchor path pool are sized by what the stream's batches have used, not by every slot's worst case (a 2 000 x 50 kb batch on a 960 Mbp
		// graph has 21 M slots: 26 GB of trace pool by worst case); a batch that needs more than its stream has seen so far runs its fragment pipeline again with the room it asked for
		while (fragmentPoolsOverflowed()) { fragmentPipeline(); resultsBack(); stageDone(3); }
		res->counters[6] = poolReruns;
		compactAnchors(); stageDone(4);
		stitchAndChainDistances(); stageDone(5);
		pass.join(tJoined, cpuJoined); stageDone(6);
		chainedAlignments(); stageDone(7);
		output.choose(stream); stageDone(8);
		assemble(); stageDone(9);
		st->fragShare = (double)res->counters[4] / (double)std::max<uint64_t>(1, R->totalBases);
		st->batchesDone++;
		if (cpuStages)
			fprintf(stderr, "[gc cpu] main thread, ms of its own CPU: seeds %.1f, whole-read set-up %.1f + start %.1f, fragment pipeline %.1f, results back %.1f, stitching + chain distances %.1f, join %.1f, chained alignments %.1f, output %.1f, assembly %.1f; pass thread %.1f\n",
				cpuStage[0], cpuStage[1], cpuStage[2], cpuStage[3], cpuStage[4], cpuStage[5], cpuStage[6], cpuStage[7], cpuStage[8], cpuStage[9], pass.passCpuMs());
		if (cpuStages)   // (with one batch in flight: this call's own; the pool's figure includes this thread's share of the jobs, which the line above counts too)
			fprintf(stderr, "[gc cpu] worker pool jobs, ms of CPU over all threads, by stage: %.1f %.1f %.1f %.1f %.1f %.1f %.1f %.1f %.1f %.1f; the process in all %.1f\n",
				poolStage[0], poolStage[1], poolStage[2], poolStage[3], poolStage[4], poolStage[5], poolStage[6], poolStage[7], poolStage[8], poolStage[9], processCpuMs() - processAt);
	}

#include "batch/gc_batch_seeds.inc"   // K1 seed lookup and the glue between it and the extension kernels
#include "batch/gc_batch_fragments.inc"   // the fragment pipeline: windows, work items, extension and anchors in lazy rounds, chaining, stitching
#include "batch/gc_batch_results.inc"   // what comes down: anchors, chains, stitched paths, the chains' NW distances
#include "batch/gc_batch_output.inc"   // the chained alignments' traces, the flat result
};

// The extension block's checks (src/AlignerMain.cpp:300-322,443-448; getSlices' assertion, ...Banded.h:504): host only, nothing but the two structs is read
static int resolveExt(const gc_params* P, const gc_params_ext* X, ClipOptions& clip)
{
	clip = ClipOptions();
	if (!X) return GC_OK;
	if (X->struct_size < sizeof(gc_params_ext)) return fail(GC_ERR_INVALID, "gc_params_ext::struct_size is smaller than the struct (was it initialised with gc_params_ext_default?)");
	if (X->struct_size > sizeof(gc_params_ext)) return fail(GC_ERR_INVALID, "gc_params_ext::struct_size is larger than this library knows: the caller's header is newer");
	if (X->x_drop < 0) return fail(GC_ERR_INVALID, "gc_params_ext::x_drop must be 0 (off) or >= 1 (src/AlignerMain.cpp:316-322)");
	const double c = X->precise_clipping;
	if (std::isnan(c) || (c != 0 && !(c >= 0.001 && c <= 0.999))) return fail(GC_ERR_INVALID, "gc_params_ext::precise_clipping must be 0 (off) or in [0.001, 0.999] (src/AlignerMain.cpp:300-315)");
	if (X->x_drop > 0 && P->force_global != 0) return fail(GC_ERR_INVALID, "gc_params_ext::x_drop cannot be combined with force_global (getSlices asserts, src/GraphAlignerBitvectorBanded.h:504)");
	clip.cutoff = c;
	clip.xDrop = X->x_drop;
	if (clip.xDrop > 0 && clip.cutoff == 0) clip.cutoff = 0.66;   // the reference's default, not an override (src/AlignerMain.cpp:443-448)
	if (clip.on()) clip.errorCost = clip.cutoff / (1.0 - clip.cutoff) + 1.0;
	return GC_OK;
}

static int alignBatch(const gc::Switches& sw, const gc_graph* G, const gc_seeder* S, const gc_seeds* H, gc_stream* st, const gc_reads* R, const gc_params* P, const ClipOptions& clip, gc_result** out)
{
	if (P->split_len < 16 || P->split_len > 64 || P->split_gap < 1) return fail(GC_ERR_INVALID, "split_len must be in [16,64] (one 64-row slice per fragment extension) and split_gap >= 1");
	if (P->ramp_bandwidth < 0 || (P->ramp_bandwidth != 0 && P->ramp_bandwidth <= P->bandwidth)) return fail(GC_ERR_INVALID, "ramp_bandwidth must be 0 (off) or larger than bandwidth (src/AlignerMain.cpp:380-383)");
	if (P->max_cells_per_slice < -1) return fail(GC_ERR_INVALID, "max_cells_per_slice must be -1 (unlimited) or >= 0");
	if (P->force_global != 0 && P->force_global != 1) return fail(GC_ERR_INVALID, "force_global must be 0 or 1");
	if (P->colinear_chaining != 0 && P->colinear_chaining != 1) return fail(GC_ERR_INVALID, "colinear_chaining must be 0 or 1");
	if (P->colinear_chaining == 0 && !P->long_pass) return fail(GC_ERR_INVALID, "colinear_chaining == 0 needs long_pass: without chaining the whole-read pass is all there is");
	if (P->extra_heuristic != 0 && P->extra_heuristic != 1) return fail(GC_ERR_INVALID, "extra_heuristic must be 0 or 1");
	if (P->selection_method < 0 || P->selection_method > GC_SELECT_ALL) return fail(GC_ERR_INVALID, "selection_method must be one of GC_SELECT_* (0..7)");
	if (P->fast_mode != 0 && P->fast_mode != 1) return fail(GC_ERR_INVALID, "fast_mode must be 0 or 1");
	if (std::isnan(P->seed_extend_density) || (P->seed_extend_density <= 0 && P->seed_extend_density != -1)) return fail(GC_ERR_INVALID, "seed_extend_density must be -1 (all seeds) or > 0 (src/AlignerMain.cpp:405)");
	if (P->seed_extend_density != -1 && P->colinear_chaining == 1) return fail(GC_ERR_INVALID, "seed_extend_density must be -1 with colinear_chaining == 1: chaining tries all seeds (src/AlignerMain.cpp:204,449-453)");
	{
		const gc_capacities& c = P->capacity;
		if (c.reserved[0] || c.reserved[1] || c.reserved[2]) return fail(GC_ERR_INVALID, "gc_params::capacity.reserved must be 0 (was the struct initialised with gc_params_default?)");
		const int64_t v[] = { c.ext_max_items, c.ext_max_pending, c.ext_max_trace, c.long_max_items, c.long_cells_per_base, c.long_scratch_bytes, c.stitch_set_max, c.stitch_bfs_cap };
		for (int64_t x : v) if (x < 0 || x > (1ll << 40)) return fail(GC_ERR_INVALID, "gc_params::capacity: a size is negative or absurd (0 = automatic)");
		// what the consumers can hold: the tables are indexed with 32 bits, and the retry launch takes 16x the fragment sizes
		if (c.ext_max_items > (1ll << 24) || c.ext_max_pending > (1ll << 24) || c.ext_max_trace > (1ll << 24)) return fail(GC_ERR_INVALID, "gc_params::capacity.ext_*: at most 2^24 (the retry launch reserves 16x)");
		if (c.long_max_items > (1ll << 28)) return fail(GC_ERR_INVALID, "gc_params::capacity.long_max_items: at most 2^28");
		if (c.long_cells_per_base > 4096) return fail(GC_ERR_INVALID, "gc_params::capacity.long_cells_per_base: at most 4096");
		if (c.stitch_set_max > (1ll << 31) - 1 || c.stitch_bfs_cap > (1ll << 31) - 1) return fail(GC_ERR_INVALID, "gc_params::capacity.stitch_*: at most 2^31 - 1");
		if (c.long_column_store < -1 || c.long_column_store > (1ll << 31)) return fail(GC_ERR_INVALID, "gc_params::capacity.long_column_store: -1 (none), 0 (automatic) or a column count");
	}
	if (P->device_output < 0 || P->device_output > 15 || (P->device_output & 3) == 3) return fail(GC_ERR_INVALID, "gc_params::device_output: 1 or 2 (GAF pieces with = / X or with M), optionally + 4 (vg::Path bytes), + 8 (corrected reads' pieces; also alone)");
	if (P->device_output && !(P->long_pass && P->edit_distances)) return fail(GC_ERR_INVALID, "gc_params::device_output needs long_pass and edit_distances (the final alignments are what it encodes)");
	*out = nullptr;
	const double tCall = nowUs();
	const double cpuCall = processCpuMs();
	gc_result* res = (gc_result*)calloc(1, sizeof(gc_result));
	int rc = guarded([&]() {
		HIP_CHECK(hipSetDevice(st->device));   // the current device is per host thread
		// without the chained alignment's trace the decision comes from the two distances alone, which skips --E-cutoff's test of the chained alignment
		// (src/Aligner.cpp:904): with a cut-off set the traces are made whatever chain_traces says
		gc_params effective = *P;
		if (effective.chain_traces == 0 && effective.e_cutoff >= 0 && effective.stitch && effective.edit_distances) effective.chain_traces = 1;
		// coverage (gc_stream_set_coverage) counts the chained winners from their traces: the winners' traces are made whatever chain_traces says
		if (st->coverage && effective.device_output && effective.chain_traces == 0 && effective.stitch && effective.edit_distances) effective.chain_traces = 1;
		if (st->coverage && effective.device_output && (st->coverage->device != st->device || st->coverage->nIds != G->hOrigSize.size()))
			throw std::runtime_error("the stream's coverage handle was made on another device or for another graph");
		BatchRun batch(sw, G, S, H, st, R, &effective, clip, res, tCall, cpuCall);
		batch.run();
		return (int)GC_OK;
	});
	if (sw.debugTimes) fprintf(stderr, "[gc times] gc_align_batch returned after %.1f ms\n", (nowUs() - tCall) / 1e3);
	if (sw.debugTimes) fprintf(stderr, "[gc token] stream %p call returned %.1f\n", (void*)st, nowUs() / 1e3);
	if (rc != GC_OK) { gc_result_free(res); return rc; }
	*out = res;
	return GC_OK;
}

int gc_align_batch_ext(const gc_graph* G, const gc_seeder* S, gc_stream* st, const gc_reads* R, const gc_seeds* H, const gc_params* P, const gc_params_ext* X, gc_result** out)
{
	if (!P || !out) return fail(GC_ERR_INVALID, "null argument");
	ClipOptions clip;
	if (int rc = resolveExt(P, X, clip)) return rc;
	if ((S != nullptr) == (H != nullptr)) return fail(GC_ERR_INVALID, "gc_align_batch_ext takes a seeder or the caller's seeds, not both and not neither");
	if (!G || !st || !R) return fail(GC_ERR_INVALID, "null argument");
	gc::Switches sw = gc::Switches::fromEnvironment();
	if (H) {
		if (H->readOffsets != R->offsets) return fail(GC_ERR_INVALID, "gc_align_batch_seeded: the seeds were uploaded for another read batch");
		if (H->device != st->device) return fail(GC_ERR_INVALID, "gc_align_batch_seeded: the seeds live on another device than the stream");
	}
	return alignBatch(sw, G, S, H, st, R, P, clip, out);
}

int gc_align_batch(const gc_graph* G, const gc_seeder* S, gc_stream* st, const gc_reads* R, const gc_params* P, gc_result** out)
{
	if (!G || !S || !st || !R || !P || !out) return fail(GC_ERR_INVALID, "null argument");
	return gc_align_batch_ext(G, S, st, R, nullptr, P, nullptr, out);
}

int gc_align_batch_seeded(const gc_graph* G, gc_stream* st, const gc_reads* R, const gc_seeds* H, const gc_params* P, gc_result** out)
{
	if (!G || !st || !R || !H || !P || !out) return fail(GC_ERR_INVALID, "null argument");
	return gc_align_batch_ext(G, nullptr, st, R, H, P, nullptr, out);
}

} // extern "C"
