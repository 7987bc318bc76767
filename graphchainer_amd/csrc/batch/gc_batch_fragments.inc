// gc_batch.hip, stage by stage (r6: one file of 2 000 lines before): the fragment pipeline: windows, work items, extension and anchors in lazy rounds, chaining, stitching.
// Member functions of struct BatchRun - this file is included INSIDE the struct's body (gc_batch.hip), which holds the members, the constructor and run().
	// ---------------- fragment windows, k_build_fragment_work, K3 / K3b in lazy rounds, K4, k_stitch - queued on the main stream
	void fragmentPipeline()
	{
		double tLongStarted = nowUs();
		if (2 * nSlots >= 0xffffffffull) throw std::runtime_error("batch too large: more than 2^31 fragment seeds; split the batch");
		if (!poolsSized) {
			traceWorst = traceBudget + traceBudget / 4 + (1u << 20);   // every slot's two extensions at full length + room for the extensions that only fit the retry launch's larger trace buffers
			pathWorst = nSlots * 24 + 4096;
			// by use: what the stream's earlier batches needed per slot, with 15 % of slack; a
			// stream's first batch starts from a low guess (60 trace cells - 8 bytes each since r6, and reserved by rows + 1 + score per extension - and 4 path words per slot of the 103 and 24 the worst case reserves) and
			// runs its fragment pipeline again with what it asked for when that was short - in the warm-up batch, once per stream - so that the pools are never larger than a batch needs
			double traceGuess = 60.0, pathGuess = 4.0, slackCells = (double)(1u << 20), slackWords = 4096.0;
			if (sw.testPoolFirstGuess) { traceGuess = *sw.testPoolFirstGuess; pathGuess = traceGuess / 8; slackCells = slackWords = 64; }   // test hook: a stream's first batch outgrows its pools
			traceBudget = std::min<uint64_t>(traceWorst, (uint64_t)((double)nSlots * (st->traceCellsPerSlot > 0 ? st->traceCellsPerSlot * 1.15 : traceGuess) + slackCells));
			pathCapacity = std::min<uint64_t>(pathWorst, (uint64_t)((double)nSlots * (st->pathWordsPerSlot > 0 ? st->pathWordsPerSlot * 1.15 : pathGuess) + slackWords));
			poolsSized = true;
		}
		ChainCaps caps { 1, 1, 1, 1 };
		caps.capAnchors = std::max(1u, maxSlotsPerRead);
		caps.capEndpoints = (uint32_t)std::min<uint64_t>(0x7fffffffull, (uint64_t)caps.capAnchors * G->maxPathsPerNode);   // entries: one per path through an anchor's end node
		caps.capTable = std::max(1u, G->maxMpcWidth);
		caps.capBack = (uint32_t)std::min<uint64_t>(0x7fffffffull, (uint64_t)caps.capAnchors * ((uint64_t)G->maxBackPerNode + G->maxPathsPerNode));   // threshold lists: backward links + paths of the start node
		res->host_us[0] = nowUs() - tGlue;
		if (sw.debugTimes) fprintf(stderr, "[gc cpu] %.0f ms of process CPU up to the end of the seed glue and the pools' sizing\n", processCpuMs() - cpuCall);
		if (sw.debugTimes) fprintf(stderr, "[gc times] seed expand+order %.1f ms, whole-read setup %.1f ms, fragment windows+arrays %.1f ms\n", (tOrdered - tGlue) / 1e3, (tLongStarted - tOrdered) / 1e3, (nowUs() - tLongStarted) / 1e3);

		// ---------------- K3 / K3b / K4
		tDev = nowUs();
		evIdx = 2;                                   // (this stage may run twice: see fragmentPoolsOverflowed)
		launchZeroWords(stream, dCursors + 1, 2);   // [1] trace pool cursor, [2] anchor path pool cursor ([0] is the seed lookup's)
		launchZeroWords(stream, dCounters, 8);
		ExtendConfig cfg;
		cfg.bandwidth = P->bandwidth;
		// --ramp-bandwidth: a fragment extension is ONE slice (split_len <= 64 rows), and slice 0 always runs with the ramp bandwidth; the rewind needs an earlier
		// slice to return to, so it never fires. An extension with the ramp on is exactly an extension at the ramp bandwidth, the slice's stored bandwidth
		// (which the backtrace reads) included (src/GraphAlignerBitvectorBanded.h:544,572-576,608). --tangle-effort goes to the cores as it is.
		if (P->ramp_bandwidth > P->bandwidth) cfg.bandwidth = P->ramp_bandwidth;
		cfg.maxCells = P->max_cells_per_slice < 0 || P->max_cells_per_slice >= 0xffffffffll ? ~0u : (uint32_t)P->max_cells_per_slice;   // (no slice reaches 2^32 - 1 cells)
		cfg.forceGlobal = P->force_global != 0;
		clip.apply(cfg);   // precise clipping / the X-drop: every extension runs in k_extend_slab_clip (below)
		cfg.maxSlices = 3;
		cfg.maxItems = 72;
		cfg.maxPending = 48;
		cfg.maxTrace = 192;
		cfg.maxItems = (uint32_t)std::max<int64_t>(8, capacityOr(sw.testExtMaxItems, P->capacity.ext_max_items, cfg.maxItems));
		cfg.maxPending = (uint32_t)std::max<int64_t>(8, capacityOr(sw.testExtMaxPending, P->capacity.ext_max_pending, cfg.maxPending));
		cfg.maxTrace = (uint32_t)std::max<int64_t>(64, capacityOr(sw.testExtMaxTrace, P->capacity.ext_max_trace, cfg.maxTrace));
		nWork = (uint32_t)(2 * nSlots);
		uint64_t slabBytes = extendSlabBytes(cfg);
		uint32_t lanes = extendGridLanes(nWork);
		ExtItem* dWork = st->work.reserve<ExtItem>(nWork);
		dResults = st->results.reserve<ExtResult>(nWork);
		// r6: fragments of up to 65 bases (one slice per extension) go through the lockstep kernel (gc_extend_frag.hip); what it declines and every longer fragment through the
		// plain-layout kernel on per-lane slabs. GC_EXTEND_SLAB=1: the plain-layout kernel for everything, as up to r5 (A/B)
		const bool fragKernel = P->split_len <= 65 && !sw.extendSlab && !clip.on();   // (the lockstep kernel does not clip: a clipped batch takes the path of its declined items for everything)
		uint8_t* dScratch = fragKernel ? nullptr : st->scratch.reserve<uint8_t>((uint64_t)lanes * slabBytes);
		const uint32_t fragWaves = fragKernel ? extendFragWaves() : 0;
		uint4* dFragItems = fragKernel ? st->fragItems.reserve<uint4>(extendFragScratchBytes(fragWaves) / sizeof(uint4)) : nullptr;
		uint32_t* dFragRetry = fragKernel ? st->fragRetryList.reserve<uint32_t>(std::max<uint32_t>(1, nWork)) : nullptr;
		unsigned long long* dFragClaims = st->fragClaims.reserve<unsigned long long>(16);   // ([8..15]: the profiling build's section cycles)   // per extension round: [2 k] the waves' claim cursor, [2 k + 1] the number of declined items
		if (fragKernel) launchZeroWords(stream, dFragClaims, 16);
		unsigned long long* hFragDeclined = st->hFragDeclined.reserve<unsigned long long>(1);
		const FragReads fragReads { R->devMasks, R->devMaskOff, R->devMaskWords, R->devOffsets, R->totalBases };
		if (st->poolsRerun && poolReruns == 0) {   // (the batch after a rerun: see DeviceBuffer::shrinkTo)
			st->tracePool.shrinkTo(traceBudget * sizeof(PoolCell), sw.testPoolShrinkFloor);
			st->pathPool.shrinkTo(pathCapacity * sizeof(uint32_t), sw.testPoolShrinkFloor);
			st->poolsRerun = false;
		}
		dTrace = st->tracePool.reserve<PoolCell>(traceBudget, true);
		FragSeed* dFragSeeds = st->fragSeeds.reserve<FragSeed>(nSlots);
		dAnchors = st->anchors.reserve<AnchorRec>(nSlots);
		dFragStatus = st->fragStatus.reserve<uint32_t>(nFrags);
		dFragExtended = st->fragExtended.reserve<uint32_t>(nFrags);
		dReadTies = st->readTies.reserve<uint32_t>(n);
		if (n) HIP_CHECK(hipMemsetAsync(dReadTies, 0, n * sizeof(uint32_t), stream));
		dPathPool = st->pathPool.reserve<uint32_t>(pathCapacity, true);
		dChainOut = st->chainOut.reserve<uint32_t>(nSlots);
		dChainLen = st->chainLen.reserve<uint32_t>(n);
		dChainScore = st->chainScore.reserve<unsigned long long>(n);
		dChainStatus = st->chainStatus.reserve<uint32_t>(n);
		uint32_t fewestSlots = 0xffffffffu;
		for (uint64_t r = 0; r < n; r++) fewestSlots = std::min(fewestSlots, jobs[r].nSlots);
		if (!n) fewestSlots = 0;
		const bool forceChainScratch = sw.testChainForceScratch;
		// both launches index the scratch by block (the LDS launch keeps its threshold lists there); a batch of long reads has no LDS launch
		uint32_t chainBlocks = chainLdsLaunch(fewestSlots, forceChainScratch) ? std::max(chainGridBlocks((uint32_t)n), chainScratchBlocks((uint32_t)n)) : chainScratchBlocks((uint32_t)n);
		uint8_t* dChainScratch = st->chainScratch.reserve<uint8_t>((uint64_t)std::max(1u, chainBlocks) * chainScratchBytes(caps));
		// Lazy extension (default): a seed is extended only when the reference would extend it - when it does not lie on an earlier alignment of its
		// fragment (src/GraphAligner.h:163-173). Round 0 extends every fragment's first seed; k_build_anchors parks the fragments that reach another
		// seed they must extend and queues that seed for the next round (the launches size themselves from counts on the device, no host round
		// trip); three rounds at most, the last parking round queues everything its fragments have left. On cfg2 the reference extends 47 % of the
		// seeds the windows hold. GC_EXT_LAZY=0: every seed is extended up front.
		const bool lazyExtend = sw.extLazy && nFrags > 0;
		launchBuildFragmentWork(stream, G->dev, dFrags, dFragFirstSeed, (uint32_t)nFrags, dReadSeeds, R->devOffsets, R->totalBases, (uint32_t)P->split_len, dFragSeeds, dWork, lazyExtend ? dResults : nullptr);
		mark();   // 2
		// extensions that outgrew their slab (a dense variant cluster: more tiles, queue entries or trace cells than the common case is sized
		// for) run again in a small grid with 16x the room; lanes whose items are fine only read the status array. What overflows even
		// that is flagged per read (capacity_exceeded), never a failed call.
		ExtendConfig big = cfg;
		auto times16 = [](uint32_t v) { return (uint32_t)std::min<uint64_t>(16ull * v, 0xffffffffull); };   // (saturating: the GC_EXT_* variables are not range-checked like gc_params::capacity)
		big.maxItems = times16(cfg.maxItems); big.maxPending = times16(cfg.maxPending); big.maxTrace = times16(cfg.maxTrace); big.maxSlices = cfg.maxSlices;
		if (sw.testExtRetryMaxItems) big.maxItems = *sw.testExtRetryMaxItems;   // test hook: make the retry overflow too
		const uint32_t retryLanes = 2048;
		uint8_t* dRetryScratch = st->scratchRetry.reserve<uint8_t>((uint64_t)retryLanes * extendSlabBytes(big));
		// (r5: every round's extension launches and every k_build_anchors launch sit between an event pair of their own - r4 bracketed "round 0's extensions" and "everything up to
		// the chaining kernel", so the later rounds' k_extend launches were charged to the anchors stage and roofline_other did not follow from the kernel trace)
		nExtendPairs = nAnchorPairs = 0;
		uint32_t nExtendRounds = 0;
		auto extendRound = [&](const ExtSelection& sel) {
			if (nExtendPairs < 4) HIP_CHECK(hipEventRecord(st->fragEv[2 * nExtendPairs], stream));
			if (fragKernel) {
				unsigned long long* claims = dFragClaims + 2 * (nExtendRounds++ & 3u);
				if (nExtendRounds > 4) launchZeroWords(stream, claims, 2);
				launchExtendFrag(stream, G->dev, G->devTables, cfg.bandwidth, dWork, nWork, fragReads, dResults, dFragItems, fragWaves, dTrace, dCursors + 1, traceBudget, dCounters, sel, claims, dFragRetry, claims + 1, dFragClaims + 8, cfg.maxCells, cfg.forceGlobal != 0);
				ExtSelection declined;
				declined.mode = 2; declined.list = dFragRetry; declined.listCount = claims + 1;
				// What the kernel declined (233 of cfg2's 4.4 M extensions) goes to the plain-layout kernel on the large slabs - when there is anything: its count comes to the host
				// first. A launch of that kernel with nothing to do still waits 2-7 ms for a SIMD to free a quarter of its registers beside the whole-read kernel's resident waves
				// (`gpurun_out/r6_f`: 12 ms per batch for six near-empty launches), the round trip costs the batch a few tens of microseconds while the other batches' kernels run
				HIP_CHECK(hipMemcpyAsync(hFragDeclined, claims + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
				syncStream(stream);
				if (*hFragDeclined > 0)
					launchExtend(stream, G->dev, G->devTables, G->devIupac, big, dWork, nWork, R->devBases, dResults, dRetryScratch, extendSlabBytes(big), dTrace, dCursors + 1, traceBudget, dCounters, EXT_OVERFLOW, retryLanes, declined);
			} else {
				launchExtend(stream, G->dev, G->devTables, G->devIupac, cfg, dWork, nWork, R->devBases, dResults, dScratch, slabBytes, dTrace, dCursors + 1, traceBudget, dCounters, 0, 4096, sel);
				launchExtend(stream, G->dev, G->devTables, G->devIupac, big, dWork, nWork, R->devBases, dResults, dRetryScratch, extendSlabBytes(big), dTrace, dCursors + 1, traceBudget, dCounters, EXT_OVERFLOW, retryLanes, sel);
			}
			if (nExtendPairs < 4) { HIP_CHECK(hipEventRecord(st->fragEv[2 * nExtendPairs + 1], stream)); nExtendPairs++; }
		};
		auto anchorsTimed = [&](const AnchorRounds& ar) {
			if (nAnchorPairs < 4) HIP_CHECK(hipEventRecord(st->fragEv[8 + 2 * nAnchorPairs], stream));
			launchBuildAnchors(stream, G->dev, dFrags, (uint32_t)nFrags, dFragSeeds, dResults, dTrace, P->split_len, dAnchors, dFragStatus, dFragExtended, dPathPool, dCursors + 2, pathCapacity, ar, dReadTies);
			if (nAnchorPairs < 4) { HIP_CHECK(hipEventRecord(st->fragEv[8 + 2 * nAnchorPairs + 1], stream)); nAnchorPairs++; }
		};
		if (!lazyExtend) {
			extendRound(ExtSelection());
			mark();   // 3
			anchorsTimed(AnchorRounds());
		} else {
			uint32_t* dLists = st->extLists.reserve<uint32_t>(2ull * nWork);           // two work lists, used in turn
			uint32_t* dPending = st->pendingFrags.reserve<uint32_t>(2ull * nFrags);     // two pending-fragment lists
			uint32_t* dFragNext = st->fragNext.reserve<uint32_t>(nFrags);
			unsigned long long* dRoundCounts = st->roundCounts.reserve<unsigned long long>(4);   // [2k] work list k, [2k+1] pending list k
			launchZeroWords(stream, dRoundCounts, 4);
			ExtSelection first;
			first.mode = 1; first.frags = dFrags; first.nFrags = (uint32_t)nFrags;
			extendRound(first);
			mark();   // 3 (round 0's extensions; the later rounds are charged to the anchors stage)
			const uint32_t nRounds = std::min<uint32_t>(maxWindowSeeds, 3);   // first seeds; the next seed each parked fragment needs; then all that is left of the few still parked
			for (uint32_t round = 0; round < nRounds; round++) {
				const uint32_t cur = round & 1u, nxt = cur ^ 1u;
				if (round > 0) {
					ExtSelection sel;
					sel.mode = 2; sel.list = dLists + (uint64_t)cur * nWork; sel.listCount = dRoundCounts + 2 * cur;
					extendRound(sel);
				}
				launchZeroWords(stream, dRoundCounts + 2 * nxt, 2);
				AnchorRounds ar;
				ar.lazy = 1; ar.round = round; ar.parkAll = round + 2 >= nRounds ? 1 : 0;
				ar.pending = dPending + (uint64_t)cur * nFrags; ar.pendingCount = dRoundCounts + 2 * cur + 1;
				ar.nextList = dLists + (uint64_t)nxt * nWork; ar.nextListCount = dRoundCounts + 2 * nxt;
				ar.nextPending = dPending + (uint64_t)nxt * nFrags; ar.nextPendingCount = dRoundCounts + 2 * nxt + 1;
				ar.fragNext = dFragNext;
				anchorsTimed(ar);
			}
		}
		mark();   // 4
		launchChain(stream, G->dev, dJobs, (uint32_t)n, dAnchors, dFrags, dFragStatus, P->split_len, P->split_gap, caps, dChainScratch, dChainOut, dChainLen, dChainScore, dChainStatus, sw.chainPlainScan, forceChainScratch, fewestSlots);
		mark();   // 5
		// chain stitching (src/Aligner.cpp:754-822) on the device, right behind the chaining kernel; GC_HOST_STITCH=1 keeps it on the
		// host workers (the path also taken by reads that do not fit the kernel's tables)
		deviceStitch = P->stitch && n > 0 && !sw.hostStitch;
		if (deviceStitch) {
			stitchDenseCap = stitchDenseWords(nSlots, n);
			uint32_t* dSlotOf = st->stitchSlotOf.reserve<uint32_t>(std::max<uint64_t>(1, nSlots));
			uint32_t* dRegions = st->stitchRegions.reserve<uint32_t>(stitchRegionWords(nSlots, n));
			dStitchNodes = st->stitchNodes.reserve<uint32_t>(stitchDenseCap);
			StitchInfo* dStitchInfo = st->stitchInfo.reserve<StitchInfo>(n);
			unsigned long long* dCursor = st->stitchCursor.reserve<unsigned long long>(1);
			stitchInfo = st->hStitchInfo.reserve<StitchInfo>(n);
			hStitchCursor = st->hStitchCursor.reserve<unsigned long long>(1);
			HIP_CHECK(hipMemsetAsync(dCursor, 0, sizeof(unsigned long long), stream));
			const int stitchClass = sw.stitchClass.value_or(pass.longestRead() > 16384 ? 3 : 0);
			launchStitch(stream, G->dev, dJobs, (uint32_t)n, dAnchors, dFrags, dFragStatus, dChainOut, dChainLen, dChainStatus, dPathPool, pathCapacity, (long long)P->colinear_gap, dSlotOf,
				dRegions, dStitchNodes, stitchDenseCap, dCursor, dStitchInfo,
				(uint32_t)capacityOr(sw.testStitchSetMax, P->capacity.stitch_set_max, 0), (uint32_t)capacityOr(sw.testStitchBfsCap, P->capacity.stitch_bfs_cap, 0),
				// reads beyond 16 kb: the class whose node set and wide bridge searches live in HBM scratch (r5; gc_stitch.hip) - a 50 kb read's piece holds ~2 500 split nodes, more than the
				// default class's LDS node set, and every read of config 5 used to be stitched by the host. GC_STITCH_CLASS=0 / 3 forces a class (tests, A/B)
				stitchClass, stitchClass == 3 ? st->stitchSpill.reserve<unsigned long long>((uint64_t)stitchSpillBlocks((uint32_t)n) * stitchSpillWordsPerBlock()) : nullptr);
			HIP_CHECK(hipMemcpyAsync(stitchInfo, dStitchInfo, n * sizeof(StitchInfo), hipMemcpyDeviceToHost, stream));
			HIP_CHECK(hipMemcpyAsync(hStitchCursor, dCursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		}

	}

	// the stream learns what its batches use of the two pools; true: this batch needed more than it was given (and less than the worst case): sized again, the stage runs again
	bool fragmentPoolsOverflowed()
	{
		const uint64_t traceNeed = hSmall[1], pathNeed = hSmall[2];
		const bool traceShort = traceNeed > traceBudget && traceBudget < traceWorst, pathShort = pathNeed > pathCapacity && pathCapacity < pathWorst;
		// what the stream learns is a run's use when the pool held it: the cursor of a run that overflowed also counts the requests of the retry launch, which runs every refused
		// extension again (config 5 at 960 Mbp learned 44 cells per slot from such a run where 36 are used: 2.4 GB per batch in flight)
		if (nSlots && !traceShort) st->traceCellsPerSlot = std::max(st->traceCellsPerSlot, (double)std::min(traceNeed, traceWorst) / (double)nSlots);
		if (nSlots && !pathShort) st->pathWordsPerSlot = std::max(st->pathWordsPerSlot, (double)std::min(pathNeed, pathWorst) / (double)nSlots);
		if (!traceShort && !pathShort) return false;
		// (the cursors count every request, the refused ones included - but a fragment whose extension was refused stops asking, so the need seen is a lower bound: a fifth more, and the loop comes back when that is still short)
		if (traceShort) traceBudget = std::min<uint64_t>(traceWorst, traceNeed + traceNeed / 5 + (1u << 20));
		if (pathShort) pathCapacity = std::min<uint64_t>(pathWorst, pathNeed + pathNeed / 5 + 4096);
		if (sw.debugTimes) fprintf(stderr, "[gc mem] the fragment pipeline runs again: trace pool %.2f G cells needed (now %.2f), anchor path pool %.2f G words needed (now %.2f)\n", traceNeed / 1e9, traceBudget / 1e9, pathNeed / 1e9, pathCapacity / 1e9);
		poolReruns++;
		st->poolsRerun = true;
		return true;
	}

