// The whole-read pass of a batch (K3-long, src/Aligner.cpp:630-654): set-up, the round loop, fallback reruns, selection and the NW distance of the best alignment, on a host
// thread of its own beside the batch's main thread (BatchRun, gc_batch.hip). Defined in batch/gc_long_pass.hip, a translation unit that cannot name a BatchRun member: what
// the two share is this interface.
//
// Who may touch what while the pass thread runs (between start() and join()):
// - the pass thread writes this object's members, st->longPass, res->counters_long, and of the batch's ReadGlue records the fields longAlns, longSelected,
//   longEditDistance, longFailed and capacityExceededLong; through the selectionKnown hook it runs OutputEncoder::encodeSelected (batch/gc_output_encoder.hpp), which
//   writes that object's private members and st->output; the main thread calls nothing of the encoder until join() has returned;
// - the main thread touches none of those. It reads st->batchesDone, st->fragShare, st->glue's other fields and the seeds (st->longSeeds) like the pass, and writes the first
//   two only after join().
//
// The token (one pass at a time per device slot, with the slot's scratch and round stream; gc_runtime.hpp): takeToken / dropToken work on a TokenRun that the pass thread
// creates when it starts and that dies with it. The thread releases the token itself, after its try / catch: on a failure only once the catch block has waited for the round
// stream (if the pass still held it) and for longStream - a kernel of this pass may still be writing to the shared scratch, which goes to the next pass with the token.
//
// Lifetime: ~WholeReadPass joins a thread that is still running (an exception on the main thread must not leave the pass thread behind with dangling state). The hook's
// target has to outlive the thread too: BatchRun declares its OutputEncoder before its WholeReadPass, so the pass is destroyed - and its thread joined - first.
#pragma once
#include "../gc_runtime.hpp"

struct WholeReadPass {
	// res: for counters_long (and, in join(), kernel_us[4] / [5]); st: longPass, device, batchesDone, fragShare, glue (edChainRun and everything else of it untouched)
	WholeReadPass(const gc::Switches& sw, const gc_graph* G, const gc_reads* R, const gc_params* P, const ClipOptions& clip, gc_stream* st, WorkerPool& pool, gc_result* res, double tCall)
		: sw(sw), G(G), R(R), P(P), clip(clip), st(st), L(st->longPass), pool(pool), res(res), tCall(tCall), n(R->offsets.size() - 1), hg(G->host), glue(st->glue) {}
	~WholeReadPass() { joinIfRunning(); }
	WholeReadPass(const WholeReadPass&) = delete;
	WholeReadPass& operator=(const WholeReadPass&) = delete;

	// main thread. K3-long set-up: buffers and sizes, the jobs uploaded; nothing runs yet. dLongSeeds: the batch's seeds in the pass's order, nSeedsTotal of them.
	// Without gc_params::long_pass: the batch-size check and the longest read only
	void prepare(const LongSeed* dLongSeeds, uint64_t nSeedsTotal);
	// main thread. The pass gets its own host thread from here on. selectionKnown is called once, on the pass thread, when every read's selection is known and the NW kernels
	// of the best alignments have been queued (so what the hook waits for overlaps them)
	void start(std::function<void()> selectionKnown);
	// main thread. Waits for the pass thread (its after-pass stage included), rethrows what it threw, writes kernel_us[4], kernel_us[5] and counters_long[6], folds
	// capacityExceededLong into capacityExceeded and with keep_traces stages the merged traces. tJoined: when the thread had ended (without long_pass: now); cpuJoined: the
	// process's CPU time at that moment (without long_pass: unchanged)
	void join(double& tJoined, double& cpuJoined);
	void joinIfRunning() { if (longThread.joinable()) longThread.join(); }

	// ---- read-only, valid after join(); the first three also inside the hook. Without long_pass: null / zero
	const LongReadResult* results() const { return hLongResults; }              // per read: status, alignments, seeds extended
	uint64_t cellsAsked() const { return hLongSmall ? hLongSmall[0] : 0; }      // merged-trace cells the pass asked for (refused requests included: a full pool leaves it beyond cellCapacity())
	const LongCell* deviceCells() const { return dLongCells; }                  // the merged-trace cell pool
	uint64_t cellCapacity() const { return cellBudget; }                        // its capacity
	const LongCell* stagedCells() const { return longCells; }                   // keep_traces: the merged traces in pinned staging (a pageable destination made this copy 2-3 s per 10 k reads)
	double startedUs() const { return tLongWall0; }                             // when start() was called
	double passCpuMs() const { return passThreadCpuMs; }                        // GC_DEBUG_TIMES: CPU time of the pass thread
	uint64_t longestRead() const { return maxReadLen; }                         // (valid after prepare(), with or without long_pass)

private:
	// what a run of the pass thread holds of the device's token (created by the thread, see the header comment)
	struct TokenRun {
		TokenHold token;
		bool held = false;   // between take and drop (with or without a token to hold: GC_LONG_TOKEN=0 has none)
		double tBegan = 0;   // when the thread began ("[gc token]" lines)
		int device = 0;
	};
	void threadMain(int device, const std::function<void()>& selectionKnown);
	void takeToken(TokenRun& run);
	void dropToken(TokenRun& run);
	uint64_t cellBudgetFor(uint64_t perBase) const { return gc::longCellBudget(R->offsets.data(), n, perBase); }
	bool growLongCells();
	bool growAlnSlots(const std::vector<uint32_t>& reads, bool keep);
	bool growLongAlns();
	void runLongRounds(TokenRun& run);
	uint64_t longFallback();
	void decideLongReads(hipStream_t q);
	void finishLongDecision();
	void afterLongPass(const std::function<void()>& selectionKnown);

	// ---- the call
	const gc::Switches& sw;
	const gc_graph* const G; const gc_reads* const R; const gc_params* const P; const ClipOptions clip;
	gc_stream* const st; gc_stream::LongPass& L;   // L: st->longPass
	WorkerPool& pool;
	gc_result* const res;
	const double tCall;
	const uint64_t n;                        // reads in the batch
	const gc::AlignmentGraph& hg;
	std::vector<ReadGlue>& glue;             // per-read host records (the fields named in the header comment)
	const gc::EValueModel evalueModel { clip.on() ? clip.cutoff : 0.7 };   // src/Aligner.cpp:474-482: the clipping cut-off is the model's identity
	// ---- prepare()
	const LongSeed* dLongSeeds = nullptr;
	uint32_t firstAlnCap = 0;                     // alignment slots every read starts with
	uint64_t alnSlots = 0;                        // slots of the batch: n * firstAlnCap, plus the new slots of reads that outgrew theirs (growAlnSlots)
	LongAln* hLongAlns = nullptr;
	unsigned long long* hLongSmall = nullptr;
	LongReadResult* hLongResults = nullptr;
	LongCell* dLongCells = nullptr;
	uint64_t cellBudget = 0;                      // capacity of the merged-trace cell pool (grown and the pass rerun when a batch overflows it)
	unsigned long long* longScratchOfToken = nullptr;   // the device's shared extension scratch, set by the pass once it holds the token
	// r4: the token is taken when the pass's FIRST extension kernel is about to be queued and given back when the last round's count (zero) has come down: a pass's first
	// init / select / order / publish and the host's wait for the work count (each a launch that queues among the other batches' kernels), and its k_long_finish at the
	// end, no longer sit between two passes' extension kernels
	RoundStream* passRounds = nullptr;   // between take and drop: the round loop's stream and events - the token slot's, or the gc_stream's own without a token (GC_LONG_TOKEN=0)
	uint64_t longScratchWords = 0;
	bool shareLongScratch = false;
	double longExtendUs = 0; uint32_t longRounds = 0;   // the rounds' extension kernels (event pairs) and how many rounds had work, reruns of the pass included
	struct DecisionPointers { EdPair* hPairs = nullptr; int64_t* hOut = nullptr; EdPair* dPairs = nullptr; int64_t* dOut = nullptr; char* dLetters = nullptr; uint32_t* dLettersLen = nullptr; } decisionPtr;
	// ... the pass's own buffers and sizes (prepare sets them; runLongRounds / growLongCells / longFallback / afterLongPass run on the pass thread)
	LongJob* hJobs = nullptr;
	bool cellPoolPinned = 0;
	uint64_t waveWords = 0;
	LongJob* dLongJobs = nullptr;
	LongAln* dLongAlns = nullptr;
	uint32_t cursorWords = 0;
	uint64_t workCapacity = 0;       // entries of the rounds' work arrays
	uint64_t roundTraceBudget = 0;   // words of the rounds' trace pool
	unsigned long long* dLongCursor = nullptr;
	LongState* dLongState = nullptr;
	LongWork* dLongWork = nullptr;
	LongWorkResult* dLongWorkResults = nullptr;
	uint32_t* dCandSeed = nullptr;
	uint32_t* dWorkLen = nullptr;
	uint32_t* dRetryList = nullptr;
	uint32_t* dOrder = nullptr;
	unsigned long long* dRoundTrace = nullptr;
	uint64_t scratchLanes = 0;
	hipStream_t ls = nullptr;
	ExtendConfig lcfg;
	unsigned long long* dLongScratchOwn = nullptr;   // (this stream's own scratch: only without the one-pass-at-a-time token)
	uint64_t maxReadLen = 1;
	// ---- start()
	std::thread longThread;
	double passThreadCpuMs = 0;   // (read after the join)
	std::exception_ptr longError;
	double tLongWall0 = 0;
	double longWallBeginUs = 0.0;   // when the pass first got the device's token (waiting for another batch's pass is not its own time; 0: not yet); written by the pass thread, read after the join
	double longWallEndUs = 0.0;     // when it last gave the token back
	// ---- join()
	const LongCell* longCells = nullptr;
};
