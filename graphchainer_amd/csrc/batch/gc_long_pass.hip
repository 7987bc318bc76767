// The whole-read pass (struct WholeReadPass, batch/gc_long_pass.hpp): set-up, the round loop, fallback reruns, selection and NW distance, its own host thread. Host code only:
// the kernels are hip/gc_long_rounds.hip and hip/gc_long_extend*.hip, the sizing and growth rules host/gc_long_policy.hpp.
#include "gc_long_pass.hpp"

// ---------------- K3-long set-up: buffers, the round loop (runLongRounds), the rerun rules; nothing runs yet
void WholeReadPass::prepare(const LongSeed* dLongSeedsOfBatch, uint64_t nSeedsTotal)
{
	// ---------------- K3-long: whole-read pass on its own stream (src/Aligner.cpp:630-654)
	dLongSeeds = dLongSeedsOfBatch;
	uint64_t nLongSeeds = 0;
	maxReadLen = 1;
	for (uint64_t r = 0; r < n; r++) maxReadLen = std::max<uint64_t>(maxReadLen, R->offsets[r + 1] - R->offsets[r]);
	firstAlnCap = gc::longFirstAlnCap(maxReadLen);   // (32, or more for long reads; a read that needs more runs again with four times the slots, growAlnSlots)
	if (sw.testLongMaxAlignments) firstAlnCap = *sw.testLongMaxAlignments;   // test hook: a tiny first capacity, so that ordinary reads take the rerun too
	alnSlots = n * (uint64_t)firstAlnCap;
	if (P->long_pass && alnSlots >= 0xffffffffull) throw std::runtime_error("batch too large for the whole-read pass");
	// Decision for a set of reads whose whole-read alignments are final: the reference's alignment order, the GreedyLength
	// selection, and (queued, not awaited) the path letters + NW edit distance of the best alignment. (Tried: deciding the
	// reads that are already finished when the rounds turn latency-bound, so these kernels run beside the last rounds - the
	// rounds slow down by more than the 11 ms the tail saves: 304-319 -> 318-337 ms per batch. So: all reads, after the rounds.)
	if (P->long_pass) {
		nLongSeeds = nSeedsTotal;   // (the glue's seed lists sit at the reads' capacity offsets)
		if (nLongSeeds >= 0xffffffffull) throw std::runtime_error("batch too large for the whole-read pass");
		hJobs = L.hLongJobs.reserve<LongJob>(n);
		// merged-trace cells per read base: 8 hold the few partial alignments a 10 kb ONT read collects before its end-to-end one (cfg2 uses ~1.1);
		// noisy 50 kb CLR reads on a genome with repeats collect 8-9 alignments each and overflowed it (a quarter of the reads flagged, which reads
		// depending on timing). The stream remembers what its batches needed, and a batch that overflows reruns its pass with three times the room.
		cellPoolPinned = sw.testLongCellsPerBase || P->capacity.long_cells_per_base > 0;
		uint64_t cellsPerBase = (uint64_t)std::max<int64_t>(2, capacityOr(sw.testLongCellsPerBase, P->capacity.long_cells_per_base, (int64_t)L.longCellsPerBase));
		if (sw.testLongForceFallback && !cellPoolPinned) cellsPerBase *= 3;   // (test hook: every read's alignments are made twice, by the rounds and by the fallback kernel, into the same pool)
		cellBudget = cellBudgetFor(cellsPerBase);
		pool.run(n, [&](size_t r, size_t) {
			const ReadGlue& gl = glue[r];
			LongJob& j = hJobs[r];
			j.maskOff = R->maskOff[r];
			j.maskWords = R->maskWords[r];
			j.alnCap = firstAlnCap;
			j.readOff = R->offsets[r];
			j.readLen = (uint32_t)(R->offsets[r + 1] - R->offsets[r]);
			j.seedBegin = (uint32_t)gl.longSeedBegin;
			j.seedEnd = (uint32_t)(gl.longSeedBegin + gl.nSeedsR);
			j.alnBegin = (uint32_t)(r * firstAlnCap);
			// size_t extendSeeds = seedExtendDensity * sequence.size() + 1, in double and then truncated; -1: the read's seed count (src/GraphAligner.h:121-122)
			j.extendSeeds = j.seedEnd - j.seedBegin;
			if (P->seed_extend_density != -1) j.extendSeeds = (uint32_t)std::min<double>(4294967295.0, P->seed_extend_density * (double)j.readLen + 1);
			j.pad = 0;
		});
		lcfg.bandwidth = P->bandwidth;
		lcfg.rampBandwidth = P->ramp_bandwidth;
		lcfg.maxCells = P->max_cells_per_slice < 0 || P->max_cells_per_slice >= 0xffffffffll ? ~0u : (uint32_t)P->max_cells_per_slice;   // (no slice reaches 2^32 - 1 cells)
		const bool globalOrClip = P->force_global || clip.on();
		const gc::LongExtendSizes sizes = gc::longExtendSizes(maxReadLen, globalOrClip);
		lcfg.maxSlices = sizes.maxSlices;
		lcfg.maxItems = sizes.maxItems;
		lcfg.maxPending = sizes.maxPending;
		lcfg.forceGlobal = P->force_global != 0;
		lcfg.maxTrace = sizes.maxTrace;
		clip.apply(lcfg);   // precise clipping / the X-drop: the rounds launch k_long_extend<.., true, true>, the fallback k_long_pass<true, true>
		lcfg.maxCols = (uint32_t)std::max<int64_t>(0, capacityOr(sw.testLongMaxCols, P->capacity.long_column_store, sizes.defaultCols));   // the column store (-1 in the parameters, 0 in the environment: no store)
		lcfg.maxItems = (uint32_t)std::max<int64_t>(64, capacityOr(sw.testLongMaxItems, P->capacity.long_max_items, lcfg.maxItems));
		if (sw.testLongRegCap) lcfg.regCap = *sw.testLongRegCap;   // test hook: force the LDS-table retry
		waveWords = longWaveWordsPerLane(lcfg);
		dLongJobs = L.longJobs.reserve<LongJob>(n);
		dLongAlns = L.longAlns.reserve<LongAln>(alnSlots);
		LongReadResult* dLongResults = L.longResults.reserve<LongReadResult>(n);
		dLongCells = L.longCells.reserve<LongCell>(cellBudget, true);
		// the rounds are serial (select -> extend -> merge, the host decides when to stop) and have a stream of their own beside the pass's stream: the token slot's
		// (takeToken sets passRounds); what comes before the token - init and the first round's select - runs on the pass's stream
		// cursors: [0] cell pool, [8..15] counters (+ [16..31] profiling stamps), the round loop's at [32..35]: work count, round trace cursor, next work slot, length of the retry list
		cursorWords = 32 + 8 * 16;
		dLongCursor = L.longCursor.reserve<unsigned long long>(cursorWords);
		hLongAlns = L.hLongAlns.reserve<LongAln>(alnSlots);
		hLongResults = L.hLongResults.reserve<LongReadResult>(n);
		hLongSmall = L.hLongSmall.reserve<unsigned long long>(cursorWords);
		ls = L.longStream;
		HIP_CHECK(hipMemsetAsync(dLongCursor, 0, cursorWords * sizeof(unsigned long long), ls));
		if (n) HIP_CHECK(hipMemcpyAsync(dLongJobs, hJobs, n * sizeof(LongJob), hipMemcpyHostToDevice, ls));
		syncStream(ls);   // the round stream starts from uploaded inputs
		// rounds: select -> extend -> merge until no read has a seed left to extend (see gc_long_rounds.hip, "K3-long in rounds")
		dLongState = L.longState.reserve<LongState>(n);
		workCapacity = gc::longWorkCapacity(n);
		dLongWork = L.longWork.reserve<LongWork>(workCapacity);
		dLongWorkResults = L.longWorkResults.reserve<LongWorkResult>(workCapacity);
		dCandSeed = L.longCandSeed.reserve<uint32_t>(2 * workCapacity);   // (the rounds use the first half; the size is as it has been)
		dWorkLen = L.longWorkLen.reserve<uint32_t>(workCapacity);   // written by k_long_select, sorted into dOrder by k_long_order: the host only
		dRetryList = L.longRetryList.reserve<uint32_t>(workCapacity);   // work items whose band outgrew the register tables (per round)
		dOrder = L.longOrder.reserve<uint32_t>(workCapacity);       // learns the round's work count (k_publish: no copy-engine transfer in the round loop)
		roundTraceBudget = gc::longRoundTraceBudget(R->offsets.data(), n, globalOrClip);   // up to four candidate seeds' worth per read
		dRoundTrace = L.longRoundTrace.reserve<unsigned long long>(roundTraceBudget);
		// extension scratch: one region per lane of a resident wave (persistent waves fetch work items)
		// (bounded by a memory budget: 0.8 MB per lane for 10 kb reads, 2.4 MB for 50 kb reads; GC_TEST_LONG_SCRATCH_GB overrides the 48 GB)
		uint64_t scratchBudget = P->capacity.long_scratch_bytes > 0 ? (uint64_t)P->capacity.long_scratch_bytes : (48ull << 30) / (uint64_t)longTokenCount(sw.longTokens, n, st->batchesDone, st->fragShare);
		if (sw.testLongScratchGb) scratchBudget = *sw.testLongScratchGb << 30;
		scratchLanes = gc::longScratchLanes(workCapacity, n, scratchBudget, waveWords);   // (no more lanes than a round can hold without speculation)
		// one pass at a time (the default) works in the device's shared scratch; GC_LONG_TOKEN=0 lets passes overlap, each in its stream's own
		longScratchWords = scratchLanes * waveWords;
		shareLongScratch = sw.shareLongScratch();   // (whoever holds the token owns the scratch)
		if (!shareLongScratch) dLongScratchOwn = L.longScratch.reserve<unsigned long long>(longScratchWords);
		// reads whose band did not fit the LDS tables (status 5) are rerun with the plain-layout kernel
	}
	// The whole-read pass is the longest leg of the batch: its round loop runs on its own host thread and stream from
	// here on, while this thread prepares and runs the fragment pipeline.
}

bool WholeReadPass::growLongCells()   // whole-read pass thread: the cell pool was too small -> enlarge it, reset the pass's cursors; false when it cannot grow
{
	bool overflowed = false;
	for (uint64_t r = 0; r < n && !overflowed; r++) overflowed = hLongResults[r].status == 4;
	if (!overflowed || cellPoolPinned) return false;   // (a pinned pool flags the reads instead: the caller asked for that much and no more)
	// by what the pass asked for (the pool's cursor counts every request, refused ones included), half as much again: gc::longCellsPerBaseForRerun
	HIP_CHECK(hipMemcpyAsync(hLongSmall, dLongCursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, ls));
	syncStream(ls);
	const uint64_t asked = hLongSmall[0], bases = std::max<uint64_t>(1, R->totalBases);
	const uint64_t next = gc::longCellsPerBaseForRerun(L.longCellsPerBase, asked, bases);
	if (sw.debugTimes) fprintf(stderr, "[gc mem] the whole-read pass runs again: %.2f G merged-trace cells asked for, %.2f G reserved (%llu per read base), now %llu per base\n", asked / 1e9, cellBudget / 1e9, (unsigned long long)L.longCellsPerBase, (unsigned long long)next);
	if (gc::longCellPoolRefused(next, cellBudgetFor(next), sizeof(LongCell))) return false;
	L.longCellsPerBase = next;
	cellBudget = cellBudgetFor(next);
	dLongCells = L.longCells.reserve<LongCell>(cellBudget, true);
	HIP_CHECK(hipMemsetAsync(dLongCursor, 0, cursorWords * sizeof(unsigned long long), ls));
	syncStream(ls);
	return true;
}

// Reads that found more alignments than they had slots for (status 3): each gets four times as many, in new slots behind the ones in use (the old ones are left unused),
// and runs again - after the rounds the whole pass (growLongAlns), after the plain-layout reruns those reads alone (longFallback; keep: the other reads' alignments
// are in the block and move with it). How many, and when a read is flagged instead: gc::longAlnSlotGrowth. Returns false when none of the reads can be given more.
bool WholeReadPass::growAlnSlots(const std::vector<uint32_t>& reads, bool keep)
{
	uint64_t total = alnSlots;
	std::vector<std::pair<uint32_t, uint32_t>> grown;   // (read, its new number of slots)
	for (uint32_t r : reads) {
		const std::optional<uint32_t> next = gc::longAlnSlotGrowth(hJobs[r].alnCap, hJobs[r].seedEnd - hJobs[r].seedBegin, total);
		if (!next) continue;
		grown.push_back({ r, *next });
		total += *next;
	}
	if (grown.empty()) return false;
	if (sw.debugTimes) fprintf(stderr, "[gc mem] %zu reads found more whole-read alignments than they had slots for and run again: %llu -> %llu slots in the batch\n", grown.size(), (unsigned long long)alnSlots, (unsigned long long)total);
	if (keep && total * sizeof(LongAln) > L.longAlns.bytes) L.longAlns.growKeeping<LongAln>(total, alnSlots, ls);
	dLongAlns = L.longAlns.reserve<LongAln>(total);
	uint64_t at = alnSlots;
	for (const auto& g : grown) { hJobs[g.first].alnBegin = (uint32_t)at; hJobs[g.first].alnCap = g.second; at += g.second; }
	alnSlots = total;
	HIP_CHECK(hipMemcpyAsync(dLongJobs, hJobs, n * sizeof(LongJob), hipMemcpyHostToDevice, ls));
	syncStream(ls);
	return true;
}

bool WholeReadPass::growLongAlns()   // whole-read pass thread, after the rounds: reads with status 3 get more slots and the pass's cursors are reset; false when there is nothing to grow
{
	std::vector<uint32_t> full;
	for (uint64_t r = 0; r < n; r++) if (hLongResults[r].status == 3) full.push_back((uint32_t)r);
	if (full.empty() || !growAlnSlots(full, false)) return false;
	HIP_CHECK(hipMemsetAsync(dLongCursor, 0, cursorWords * sizeof(unsigned long long), ls));
	syncStream(ls);
	return true;
}

void WholeReadPass::runLongRounds(TokenRun& run)   // the round loop: select -> extend -> merge until no read has a seed left to extend (see gc_long_rounds.hip, "K3-long in rounds")
{
	if (n == 0) return;
	unsigned long long* dLongScratch = nullptr;   // (set when the token is taken - before the first extension launch)
	hipStream_t q = ls;                           // until the token is taken: the pass's own stream; from then on the round stream of the token slot the pass holds (passRounds)
	hipEvent_t* ring = nullptr;
	// the rounds' extension time: read a ring slot's pair before the slot is reused (its round is complete by then: every round's
	// work count has been awaited since) and what is left after the last round
	auto collect = [&](int slot) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ring[2 * slot], ring[2 * slot + 1])); longExtendUs += (double)ms * 1000.0; };
	int timedRounds = 0;
	unsigned long long* cursor = dLongCursor + 32;
	volatile unsigned long long* hCursor = hLongSmall + 32;
	double dbgWaitUs = 0;
	const double dbgT0 = nowUs();
	// what comes before the token - init, the first round's select, order and publish - runs on the pass's own stream, beside the pass that holds the token now
	launchLongInit(q, dLongJobs, (uint32_t)n, dLongState);
	uint32_t lastWork = 0xffffffffu;

	for (int round = 0; round < 4096; round++) {
		launchZeroWords(q, cursor, 4);   // [0] work count, [1] round trace cursor, [2] next work slot, [3] length of the retry list
		uint32_t maxCand = gc::longCandidatesPerRead(round, lastWork, n);   // one, and several in the tail rounds
		if (sw.testLongSpeculate) maxCand = *sw.testLongSpeculate;   // test hook: speculate from round 0
		launchLongSelect(q, G->dev, dLongJobs, (uint32_t)n, dLongSeeds, R->totalBases, (uint32_t)P->min_cluster_size, (uint32_t)P->extra_heuristic, maxCand, dLongState, dLongAlns, dLongCells, dLongWork, dWorkLen, dCandSeed, cursor, workCapacity);
		// execution order: longest extensions first, so the round's tail is made of short ones (GC_TEST_LONG_ORDER=0: as emitted)
		launchLongOrder(q, dWorkLen, cursor, dOrder, (uint32_t)maxReadLen, sw.testLongOrder);
		launchPublish(q, cursor, (unsigned long long*)hCursor, 2);
		const double tWait0 = nowUs();
		syncStream(q);
		dbgWaitUs += nowUs() - tWait0;
		uint32_t nWorkItems = (uint32_t)hCursor[0];
		if (nWorkItems == 0) break;
		if (!dLongScratch) {
			// (the host has just waited for the pass's own stream: everything queued there is complete, so no event links it to the token's stream)
			takeToken(run);
			dLongScratch = shareLongScratch ? longScratchOfToken : dLongScratchOwn;
			q = passRounds->q;
			ring = passRounds->ring;
		}
		uint32_t team = longExtendTeamSize(nWorkItems, sw.testLongTeam.value_or(0));
		uint32_t blocks = gc::longRoundBlocks(nWorkItems, team, scratchLanes);
		if (sw.testLongMaxBlocks) blocks = std::min<uint32_t>(blocks, *sw.testLongMaxBlocks);   // test hook: force persistent waves
		if (timedRounds >= LONG_EVENT_RING) collect(timedRounds % LONG_EVENT_RING);
		hipEvent_t ev0 = ring[2 * (timedRounds % LONG_EVENT_RING)], ev1 = ring[2 * (timedRounds % LONG_EVENT_RING) + 1];
		HIP_CHECK(hipEventRecord(ev0, q));
		launchLongExtend(q, G->dev, G->devTables, R->devMasks, lcfg, dLongWork, dOrder, nWorkItems, dLongScratch, team, blocks,
			dRoundTrace, cursor + 1, roundTraceBudget, dLongWorkResults, dLongCursor + 8, cursor + 2, 0, nullptr, team == 1 ? dRetryList : nullptr, cursor + 3);
		if (team == 1) {
			// extensions whose band outgrew the 64-entry register tables: second try with the LDS/HBM tables (two lanes per wave,
			// 28 + 228 entries); waves whose items are fine leave at once. Beyond that the read goes to the plain-layout fallback.
			// (those items are listed first - almost always none - so that the retry is a handful of waves that fetch from the list, not
			// one wave per pair of work items that looks at a status and leaves: that cost 0.5-2 ms of every round)
			if ((uint64_t)blocks * team < nWorkItems) launchZeroWords(q, cursor + 2, 1);   // (persistent waves used the slot counter; the retry list is the extension kernel's own)
			uint32_t retryBlocks = gc::longRetryBlocks(scratchLanes);   // (persistent waves over a list that is almost always empty on 10 kb reads)
			launchLongExtend(q, G->dev, G->devTables, R->devMasks, lcfg, dLongWork, dRetryList, nWorkItems, dLongScratch, 2, retryBlocks,
				dRoundTrace, cursor + 1, roundTraceBudget, dLongWorkResults, dLongCursor + 8, cursor + 2, EXT_LDS_CAP, cursor + 3);
		}
		HIP_CHECK(hipEventRecord(ev1, q));
		launchLongMerge(q, G->dev, dLongJobs, (uint32_t)n, dLongSeeds, dCandSeed, dLongWorkResults, dRoundTrace, dLongState, dLongAlns, dLongCells, dLongCursor, cellBudget, (uint32_t)P->extra_heuristic);
		lastWork = nWorkItems;
		// no wait here: the next round's select / order / publish queue up right behind the merge, and the only host round trip per
		// round is the work count above (with a second wait after the merge the stream drained twice per round)
		timedRounds++;
		longRounds++;
	}
	// (the last round's count has come down: every extension kernel of the pass is complete, the scratch is free and the token's stream is empty)
	const double dbgT1 = nowUs();
	if (ring) for (int k = std::max(0, timedRounds - LONG_EVENT_RING); k < timedRounds; k++) collect(k % LONG_EVENT_RING);   // (before the release: the ring goes to the next pass with the token)
	dropToken(run);
	// the per-read results go straight into pinned host memory (the kernel writes them across PCIe): a copy-engine transfer here queued behind
	// the other batch's bulk downloads for 30-50 ms while this pass still held the device's whole-read token. On the pass's own stream: the token's is the next pass's now
	launchLongFinish(ls, (uint32_t)n, dLongState, hLongResults);
	syncStream(ls);
	if (sw.debugTimes) {
		const char* hwq = getenv("GPU_MAX_HW_QUEUES");
		fprintf(stderr, "[gc times] whole-read rounds: %.1f ms in all, %.1f ms waiting for the rounds' work counts, %.1f ms in the last wait, %d rounds, GPU_MAX_HW_QUEUES=%s\n", (nowUs() - dbgT0) / 1e3, dbgWaitUs / 1e3, (nowUs() - dbgT1) / 1e3, timedRounds, hwq ? hwq : "unset");
	}
}

uint64_t WholeReadPass::longFallback()   // reads whose band did not fit the wave layout's tables are rerun with the plain-layout kernel; returns how many
{
	syncStream(ls);
	std::vector<uint32_t> redo;
	const bool forceAll = sw.testLongForceFallback;   // test hook: run every read through the plain-layout kernel too
	// status 5: a slice with more nodes than the wave tables hold; status 2: an extension with more tiles / trace cells than its scratch
	// (the plain-layout kernel below gets four times the room)
	for (uint64_t r = 0; r < n; r++) if (hLongResults[r].status == 5 || hLongResults[r].status == 2 || forceAll) redo.push_back((uint32_t)r);
	if (!redo.empty()) {
		ExtendConfig fcfg = lcfg;
		fcfg.maxItems = 4 * lcfg.maxItems; fcfg.maxTrace = 2 * lcfg.maxTrace; fcfg.maxPending = 4 * lcfg.maxPending;
		uint64_t lslab = longSlabBytes(fcfg);
		// The reruns append their cells to the pool the rounds have filled, and the pool is sized by use: a rerun that finds it full answers status 4. The round loop's
		// overflow runs the pass again (growLongCells); here the pool grows IN PLACE - a larger block, the cells already written copied over - and only the reads that were
		// refused run again, in this batch (r5 flagged them and gave the room to the stream's next batch: a read's output depended on its stream's history - ADVICE r5)
		std::vector<uint32_t> now = redo;
		for (int cellGrowths = 0; !now.empty(); ) {
			std::vector<LongJob> subJobs(now.size());
			for (size_t i = 0; i < now.size(); i++) subJobs[i] = hJobs[now[i]];
			uint64_t lanes = (now.size() + 63) / 64 * 64;
			LongJob* dSubJobs = L.longJobsFallback.reserve<LongJob>(now.size());
			LongReadResult* dSubResults = L.longResultsFallback.reserve<LongReadResult>(now.size());
			uint8_t* dSlab = L.longScratchFallback.reserve<uint8_t>(lanes * lslab);
			HIP_CHECK(hipMemcpyAsync(dSubJobs, subJobs.data(), now.size() * sizeof(LongJob), hipMemcpyHostToDevice, ls));
			launchLongPass(ls, G->dev, G->devTables, G->devIupac, fcfg, dSubJobs, (uint32_t)now.size(), dLongSeeds, R->devBases, R->totalBases, (uint32_t)P->min_cluster_size, (uint32_t)P->extra_heuristic,
				dSlab, lslab, dLongCells, dLongCursor, cellBudget, dLongAlns, dSubResults, dLongCursor + 8);
			std::vector<LongReadResult> subResults(now.size());
			HIP_CHECK(hipMemcpyAsync(subResults.data(), dSubResults, now.size() * sizeof(LongReadResult), hipMemcpyDeviceToHost, ls));
			HIP_CHECK(hipMemcpyAsync(hLongSmall, dLongCursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, ls));
			syncStream(ls);
			std::vector<uint32_t> refused, full;
			for (size_t i = 0; i < now.size(); i++) {
				hLongResults[now[i]] = subResults[i];
				if (subResults[i].status == 4) refused.push_back(now[i]);
				if (subResults[i].status == 3) full.push_back(now[i]);
			}
			// reads that ran out of alignment slots here (the rounds never finished them, so nobody knew their count): more slots, and again with the refused ones
			if (!full.empty() && !growAlnSlots(full, true)) full.clear();
			if (refused.empty() || cellPoolPinned || cellGrowths >= 3) { now.swap(full); continue; }   // (a pinned pool flags the reads: the caller asked for that much and no more)
			const uint64_t used = std::min<uint64_t>(hLongSmall[0], cellBudget), next = gc::longCellsPerBaseDoubled(L.longCellsPerBase);
			if (next == L.longCellsPerBase || gc::longCellPoolRefused(next, cellBudgetFor(next), sizeof(LongCell))) { now.swap(full); continue; }
			cellGrowths++;
			if (sw.debugTimes) fprintf(stderr, "[gc mem] the plain-layout reruns of %zu reads found the merged-trace pool full: %llu -> %llu cells per read base, %.2f G cells kept\n", refused.size(), (unsigned long long)L.longCellsPerBase, (unsigned long long)next, used / 1e9);
			L.longCells.growKeeping<LongCell>(cellBudgetFor(next), used, ls, true);
			const unsigned long long cursor = used;   // (the refused requests are given back: the reruns ask again)
			HIP_CHECK(hipMemcpyAsync(dLongCursor, &cursor, sizeof(cursor), hipMemcpyHostToDevice, ls));
			syncStream(ls);
			L.longCellsPerBase = next;
			cellBudget = cellBudgetFor(next);
			dLongCells = (LongCell*)L.longCells.ptr;
			now.swap(refused);
			now.insert(now.end(), full.begin(), full.end());
		}
	}
	hLongAlns = L.hLongAlns.reserve<LongAln>(alnSlots);   // (more than prepare() reserved when reads were given more slots)
	if (n) HIP_CHECK(hipMemcpyAsync(hLongAlns, dLongAlns, alnSlots * sizeof(LongAln), hipMemcpyDeviceToHost, ls));
	HIP_CHECK(hipMemcpyAsync(hLongSmall, dLongCursor, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ls));
	syncStream(ls);
	return (uint64_t)redo.size();
}

// selection of every read's whole-read alignments and the NW distance of the best one (src/Aligner.cpp:636-654): launch ...
// (all reads, on the pool, each with the alignments its result counts: see the trial in prepare() - a subset of finished reads, decided early, lost)
void WholeReadPass::decideLongReads(hipStream_t q)
{
	// the reference re-sorts its alignment list by alignmentStart after every accepted alignment
	// (src/GraphAligner.h:183); replaying that on the acceptance-ordered list gives its final order. Then the
	// selection (host/gc_selection.hpp) with the same unstable sort.
	auto selectOne = [&](size_t i, size_t) {
		const uint32_t r = (uint32_t)i;
		ReadGlue& gl = glue[r];
		gl.longAlns.clear();
		gl.longSelected.clear();
		const uint32_t nAln = hLongResults[r].nAlignments;
		for (uint32_t a = 0; a < nAln; a++) {
			gl.longAlns.push_back(hLongAlns[(uint64_t)hJobs[r].alnBegin + a]);
			std::sort(gl.longAlns.begin(), gl.longAlns.end(), [](const LongAln& l, const LongAln& rr) { return l.start < rr.start; });
		}
		// SelectAlignments (host/gc_selection.hpp): --E-cutoff first, then GreedyLength (with chaining the whole-read side is always that, src/Aligner.cpp:636-639)
		// or gc_params::selection_method (without chaining, :927-930); the indices come in the order the reference returns the alignments
		std::vector<gc::SelectItem> items;
		for (const LongAln& al : gl.longAlns) items.push_back(gc::SelectItem { al.start, al.end, al.score });
		const size_t readLen = R->offsets[r + 1] - R->offsets[r];
		gl.longSelected = gc::selectAlignments(items, P->colinear_chaining ? (int)gc::SelectGreedyLength : (int)P->selection_method, hg.SizeInBP(), readLen, P->e_cutoff, evalueModel);
	};
	pool.run(n, selectOne);
	auto& D = L.edLong;
	D.nPairs = 0;
	D.pairRead.clear();
	if (!P->edit_distances || !P->colinear_chaining || n == 0) return;   // (without chaining the reference computes no distance: long_edit_distance stays -1)
	// edit distance of the best whole-read alignment's path against the read (edlibAlign at src/Aligner.cpp:645)
	const size_t m = n;
	PathSeqJob* hJobsPS = D.hJobs.reserve<PathSeqJob>(m);
	EdPair* hPairs = D.hPairs.reserve<EdPair>(m);
	int64_t* hOut = D.hOut.reserve<int64_t>(m);
	uint64_t nLetters = 0;
	uint32_t nPairs = 0;
	for (size_t i = 0; i < m; i++) {
		const uint32_t r = (uint32_t)i;
		const ReadGlue& gl = glue[r];
		if (gl.longSelected.empty()) { hJobsPS[i] = PathSeqJob { 0, nLetters, 0, 0, 0, 0 }; continue; }
		const LongAln& al = gl.longAlns[gl.longSelected[0]];
		uint32_t len = (uint32_t)(R->offsets[r + 1] - R->offsets[r]);
		uint32_t cap = 2 * al.traceLen + 256;
		hJobsPS[i] = PathSeqJob { al.traceOff, nLetters, al.traceLen, cap, 0, 0 };
		// the alignment itself bounds the distance: its edits plus the unaligned read ends
		hPairs[nPairs++] = EdPair { nLetters, 0, (uint32_t)i, r, al.score + al.start + (len - std::min(len, al.end)) + 8 };
		D.pairRead.push_back(r);
		nLetters += cap;
	}
	PathSeqJob* dJobsPS = D.jobs.reserve<PathSeqJob>(m);
	char* dLetters = D.letters.reserve<char>(nLetters);
	uint32_t* dLettersLen = D.lettersLen.reserve<uint32_t>(m);
	EdPair* dPairs = D.pairs.reserve<EdPair>(m);
	int64_t* dOut = D.out.reserve<int64_t>(m);
	HIP_CHECK(hipMemcpyAsync(dJobsPS, hJobsPS, m * sizeof(PathSeqJob), hipMemcpyHostToDevice, q));
	launchLongPathSeq(q, G->dev, dJobsPS, (uint32_t)m, dLongCells, dLetters, dLettersLen);
	auto readLenOf = [R = R](uint32_t r) { return (uint32_t)(R->offsets[r + 1] - R->offsets[r]); };
	launchEditDistances(D.run, q, hPairs, hOut, nPairs, dPairs, dOut, R->devEdReads, R->devBases, R->devEqMasks, dLetters, dLettersLen, readLenOf, sw.debugTimes);   // (k: the alignment's own bound)
	D.nPairs = nPairs;
	decisionPtr = DecisionPointers { hPairs, hOut, dPairs, dOut, dLetters, dLettersLen };
}

// ... and collect
void WholeReadPass::finishLongDecision()
{
	auto& D = L.edLong;
	if (!D.nPairs) return;
	const DecisionPointers& p = decisionPtr;
	finishEditDistances(D.run, L.longStream, p.hPairs, p.hOut, D.nPairs, p.dPairs, p.dOut, R->devEdReads, R->devBases, R->devEqMasks, p.dLetters, p.dLettersLen, sw.debugTimes);
	for (uint32_t i = 0; i < D.nPairs; i++) {
		ReadGlue& gl = glue[D.pairRead[i]];
		gl.longEditDistance = p.hOut[i];
		if (p.hOut[i] < -1) { gl.longEditDistance = -1; gl.capacityExceededLong = true; }   // outside the NW kernel's range: flagged, no distance
	}
	D.nPairs = 0;
}

// What follows the rounds: fallback reruns, the reference's `cont` rule, selection and the NW distance of the best whole-read alignment.
void WholeReadPass::afterLongPass(const std::function<void()>& selectionKnown)
{
	uint64_t rerun = longFallback();
	res->counters_long[7] = rerun;   // reads that needed the plain-layout fallback kernel
	for (int i = 0; i < 6; i++) res->counters_long[i] = hLongSmall[8 + i];   // same units as counters[]
#ifdef GC_STAMPS
	{
		static const char* names[11] = { "slice prologue", "pop+prev lookup", "tile columns", "item store", "edge pushes", "slice epilogue", "bt slice change", "bt item loads", "bt recompute", "bt corner", "bt walk" };
		double total = 0;
		for (int i = 0; i < 11; i++) total += (double)hLongSmall[16 + i];
		for (int i = 0; i < 11; i++) fprintf(stderr, "[gc stamps] %-16s %6.2f%%  %.3e lane-cycles\n", names[i], 100.0 * hLongSmall[16 + i] / (total > 0 ? total : 1), (double)hLongSmall[16 + i]);
	}
#endif
	if (sw.testFailLong) {   // test hook shared with the oracle: this read's whole-read pass "asserts"
		const long idx = *sw.testFailLong;
		if (idx >= 0 && (uint64_t)idx < n) hLongResults[idx].status = 1;
	}
	// A whole-read pass that trips one of the reference's live asserts leaves the read with nothing: align_fn's catch sets
	// `cont` (src/Aligner.cpp:591), which is declared once per read (:529) and makes the fragment loop skip every anchor
	// (:702-703); the alignments found before the throw are lost with the exception.
	for (uint64_t r = 0; r < n; r++) if (hLongResults[r].status == 1) { hLongResults[r].nAlignments = 0; glue[r].longFailed = true; }
	// capacities of this library, not of the reference: 2 extension scratch (even with the fallback's four-fold room), 3 more alignments than
	// LONG_ALN_SLOTS_MAX (every smaller number of slots was rerun with more, growAlnSlots), 4 the merged-trace cell pool (GC_TEST_LONG_CELLS_PER_BASE).
	// The read keeps what was found up to there and is flagged.
	for (uint64_t r = 0; r < n; r++) if (hLongResults[r].status >= 2 && hLongResults[r].status <= 4) glue[r].capacityExceededLong = true;
	decideLongReads(L.longStream);
	selectionKnown();   // (the selection is known; the hook's waits - the batch's output encoder starts here - overlap the NW kernels the decision has just queued)
	finishLongDecision();
}

// ---------------- the token: taken before the pass's first extension launch, given back when the last round's count has come down (see the header)
void WholeReadPass::takeToken(TokenRun& run)
{
	if (run.held) return;
	TokenHold& token = run.token;
	const int device = run.device;
	const bool oneAtATime = sw.onePassAtATime();   // GC_LONG_TOKEN=0: no token, passes overlap; anything else: one pass at a time
	const double tAsk = nowUs();
	if (oneAtATime) {
		const int passesSideBySide = longTokenCount(sw.longTokens, n, st->batchesDone, st->fragShare);
		token.lock(g_longPassToken[device & 15], passesSideBySide, passesSideBySide == 1);   // (a pass that fills the chip: alone on the device)
		if (token.slot > 0 && shareLongScratch) {   // the second token's scratch is only grown when the device has the room: otherwise this pass waits for the first token like any other
			const DeviceBuffer& have = g_longScratch[device & 15].buffer[token.slot];
			size_t freeBytes = 0, totalBytes = 0;
			const uint64_t need = longScratchWords * sizeof(unsigned long long);
			if (have.bytes < need && (hipMemGetInfo(&freeBytes, &totalBytes) != hipSuccess || freeBytes + have.bytes < need + need / 8 + (6ull << 30))) { token.unlock(); token.lock(g_longPassToken[device & 15], 1, false); }
		}
	}
	if (shareLongScratch && oneAtATime) {
		if (!token.owns_lock()) throw std::runtime_error("internal: shared whole-read scratch without the token");
		try {
			longScratchOfToken = g_longScratch[device & 15].buffer[token.slot].reserve<unsigned long long>(longScratchWords);
		} catch (const DeviceError&) {
			// (the check above and this reservation are not one step: another stream may have taken the memory in between) - the second token's scratch does not
			// fit after all: this pass takes its turn on the first token's instead of failing the batch
			if (token.slot == 0) throw;
			(void)hipGetLastError();
			token.unlock();
			token.lock(g_longPassToken[device & 15], 1, false);
			longScratchOfToken = g_longScratch[device & 15].buffer[0].reserve<unsigned long long>(longScratchWords);
		}
	}
	// the round loop's stream: the one of the token slot this pass now holds (every pass of the device that holds the slot runs its rounds there, one at a time);
	// without a token the gc_stream's own
	passRounds = token.owns_lock() ? &g_longScratch[device & 15].rounds[token.slot] : &L.ownRounds;
	passRounds->ensure(token.owns_lock());
	run.held = true;
	if (sw.debugTimes) fprintf(stderr, "[gc token] stream %p pass began %.1f asked %.1f got %.1f (call began %.1f)\n", (void*)st, run.tBegan / 1e3, tAsk / 1e3, nowUs() / 1e3, tCall / 1e3);
	if (longWallBeginUs == 0.0) longWallBeginUs = nowUs();   // (whole_read_pass_wall: from the pass's first take of the token - a pool rerun takes it again - to its last release)
}

void WholeReadPass::dropToken(TokenRun& run)
{
	if (!run.held) return;
	run.held = false;
	passRounds = nullptr;   // (the slot's stream goes to the next pass with the token)
	longWallEndUs = nowUs();
	if (sw.debugTimes) fprintf(stderr, "[gc token] stream %p released %.1f\n", (void*)st, nowUs() / 1e3);
	run.token.unlock();   // the next batch's pass may start; what follows is this batch's own tail
}

// ---------------- the pass gets its own host thread and stream from here on
void WholeReadPass::start(std::function<void()> selectionKnown)
{
	tLongWall0 = nowUs();
	if (P->long_pass) {
		int device = 0;
		HIP_CHECK(hipGetDevice(&device));
		longThread = std::thread([this, device, selectionKnown = std::move(selectionKnown)]() { threadMain(device, selectionKnown); });
	}
}

void WholeReadPass::threadMain(int device, const std::function<void()>& selectionKnown)
{
	// (declared outside the try block: on an exception the catch below waits for the pass's kernels BEFORE the token - and with it the device's shared scratch - is released)
	TokenRun run;
	run.device = device;
	try {
		HIP_CHECK(hipSetDevice(device));
		run.tBegan = nowUs();
		runLongRounds(run);
		while (growLongCells() || growLongAlns()) runLongRounds(run);   // the cell pool overflowed, or reads ran out of alignment slots: again, with room
		dropToken(run);
		// What follows the rounds runs here, beside the tail of the fragment pipeline (which ends 20-30 ms after the pass on cfg2, starved by it), instead of after the
		// join: 16 ms off the batch's critical path. What it may write is in the header (gc_long_pass.hpp).
		afterLongPass(selectionKnown);
		passThreadCpuMs = threadCpuMs();   // (the thread's whole life: it is created per batch)
	} catch (...) {
		longError = std::current_exception();
		// the token is released below, after these waits: a kernel of this pass may still be writing to the shared scratch
		if (passRounds && passRounds->q) (void)hipStreamSynchronize(passRounds->q);   // (still set: the pass failed between take and drop)
		passRounds = nullptr;
		(void)hipStreamSynchronize(L.longStream);
	}
	run.token.unlock();   // (after a failure: only now. Otherwise dropToken has given it back already)
}

// ---------------- the pass thread ends (its after-pass stage included)
void WholeReadPass::join(double& tJoined, double& cpuJoined)
{
	// ---------------- whole-read pass results
	tJoined = nowUs();
	if (P->long_pass) {
		double tJoin0 = nowUs();
		longThread.join();
		tJoined = nowUs();
		cpuJoined = processCpuMs();
		if (sw.debugTimes) fprintf(stderr, "[gc times] main thread waited %.1f ms for the whole-read pass\n", (tJoined - tJoin0) / 1e3);
		if (longError) std::rethrow_exception(longError);
		res->kernel_us[4] = longExtendUs;
		res->counters_long[6] = longRounds;
		res->kernel_us[5] = longWallEndUs - (longWallBeginUs > 0.0 ? longWallBeginUs : tLongWall0);   // whole-read pass, wall clock from the token to its release
		for (uint64_t r = 0; r < n; r++) if (glue[r].capacityExceededLong) glue[r].capacityExceeded = true;
		if (P->keep_traces) {
			const uint64_t cellsUsed = std::min<uint64_t>(hLongSmall[0], cellBudget);   // (the cursor counts refused requests too: a full pool leaves it beyond the pool's end)
			LongCell* staged = L.hLongCells.reserve<LongCell>(cellsUsed);
			if (cellsUsed) HIP_CHECK(hipMemcpyAsync(staged, dLongCells, cellsUsed * sizeof(LongCell), hipMemcpyDeviceToHost, L.longStream));
			syncStream(L.longStream);
			longCells = staged;
		}
	}

	if (sw.debugTimes) fprintf(stderr, "[gc times] after the whole-read pass: selection + its edit distances %.1f ms\n", (nowUs() - tJoined) / 1e3);
}
