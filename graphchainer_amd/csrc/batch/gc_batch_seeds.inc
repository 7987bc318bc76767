// gc_batch.hip, stage by stage (r6: one file of 2 000 lines before): K1 seed lookup and the glue between it and the extension kernels.
// Member functions of struct BatchRun - this file is included INSIDE the struct's body (gc_batch.hip), which holds the members, the constructor and run().
	// ---------------- K1 seed lookup, then the glue between it and the extension kernels, both on the device: the batch's seeds, fragments and chain jobs
	// are written in HBM; the host gets the counts, the per-read records and copies of what the result assembly reads
	void seeds()
	{
		// ---------------- K1: seed lookup (not with the caller's own hits, H: they were resolved when they were uploaded, and the glue starts from them)
		uint32_t* dTmp = H ? nullptr : st->tmp.reserve<uint32_t>(R->totalBases);
		uint2* dMatches = H ? nullptr : st->matches.reserve<uint2>(R->totalBases);
		uint32_t* dReadMatchOff = H ? nullptr : st->readMatchOff.reserve<uint32_t>(n);
		uint32_t* dReadMatchCount = H ? nullptr : st->readMatchCount.reserve<uint32_t>(n);
		dCursors = st->cursors.reserve<unsigned long long>(8);
		dCounters = st->counters.reserve<unsigned long long>(8);
		hSmall = st->hSmall.reserve<unsigned long long>(16);   // [0..7] cursors, [8..15] counters
		HIP_CHECK(hipMemsetAsync(dCursors, 0, 8 * sizeof(unsigned long long), stream));
		HIP_CHECK(hipMemsetAsync(dCounters, 0, 8 * sizeof(unsigned long long), stream));
		mark();   // 0
		if (!H) launchSeedLookup(stream, S->dev, R->devBases, R->devOffsets, (uint32_t)n, (uint64_t*)dCursors, dReadMatchOff, dReadMatchCount, dMatches, R->totalBases, dTmp, R->totalBases, R->devChunkRead, R->devPacked, R->devInvalid);
		mark();   // 1
		// The glue between the seed lookup and the extension kernels (hit expansion, seed ordering, fragment windows) runs on the device
		// (gc_seedglue.hip: one wave per read, the reference's three unstable sorts replayed with libstdc++'s own algorithm).
		if (glue.size() < n) glue.resize(n);
		unsigned long long* dGlueCursors = st->glueCursors.reserve<unsigned long long>(8);
		// where a read's seeds begin in the per-seed arrays: the running sum of the reads' seed bounds, or the caller's read_hit_off
		uint32_t* dSeedCap = H ? nullptr : st->glueSeedCap.reserve<uint32_t>(n);
		uint32_t* dSeedOff = H ? H->devReadHitOff : st->glueSeedOff.reserve<uint32_t>(n + 1);
		unsigned long long* hGlueSmall = st->hGlueSmall.reserve<unsigned long long>(8);
		HIP_CHECK(hipMemsetAsync(dGlueCursors, 0, 8 * sizeof(unsigned long long), stream));
		if (!H) launchSeedCaps(stream, S->dev, (uint32_t)n, R->devReadInvalid, dMatches, dReadMatchOff, dReadMatchCount, dSeedCap, dSeedOff, dGlueCursors + 5);
		HIP_CHECK(hipMemcpyAsync(hSmall, dCursors, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipMemcpyAsync(hGlueSmall, dGlueCursors, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		// capacity of the per-read window staging: one window per fragment position (host: the lengths are known)
		uint32_t* hWinCapOff = st->hGlueWinCapOff.reserve<uint32_t>(n + 1);
		uint64_t winCap = 0;
		for (uint64_t r = 0; r < n; r++) {
			const uint64_t len = R->offsets[r + 1] - R->offsets[r];
			hWinCapOff[r] = (uint32_t)winCap;
			winCap += len >= (uint64_t)P->split_len ? (len - P->split_len) / P->split_gap + 1 : 1;
		}
		hWinCapOff[n] = (uint32_t)winCap;
		if (winCap >= 0xffffffffull) throw std::runtime_error("batch too large: more than 2^32 fragment positions; split the batch");
		uint32_t* dWinCapOff = st->glueWinCapOff.reserve<uint32_t>(n + 1);
		HIP_CHECK(hipMemcpyAsync(dWinCapOff, hWinCapOff, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
		syncStream(stream);
		res->kernel_us[0] = elapsedUs(0, 1);
		res->host_us[2] = nowUs() - tTotal;   // K1 + its transfers, wall
		tGlue = nowUs();
		const uint64_t nMatchesDev = hSmall[0], seedCap = H ? H->nHits : hGlueSmall[5];
		if (nMatchesDev > R->totalBases) throw std::runtime_error("seed lookup overflowed its buffer");
		if (seedCap >= 0xfffffff0ull) throw std::runtime_error("batch too large: more than 2^32 seed occurrences; split the batch");
		nSeedsTotal = seedCap;
		GlueStaging stg;
		uint32_t** u32s[8] = { &stg.mPos, &stg.mStartLo, &stg.mStartHi, &stg.sSeqPos, &stg.sNode, &stg.sOffset, &stg.sGood, &stg.sCluster };
		for (int k = 0; k < 8; k++) *u32s[k] = H && k < 6 ? nullptr : st->glueU32[k].reserve<uint32_t>(seedCap);   // (the caller's hits: only what the glue computes per seed - goodness, cluster size)
		stg.sortBuf = (GlueElem*)st->glueSort.reserve<uint8_t>(seedCap * glueElemBytes());
		stg.sortScratch = st->gluePos.reserve<uint32_t>(3 * seedCap + 64 * n + 64);
		stg.winBuf = st->glueWin.reserve<uint32_t>(4 * winCap);
		dPassSeeds = st->longSeeds.reserve<LongSeed>(P->long_pass ? seedCap : 0);
		dReadSeeds = st->readSeeds.reserve<FragSeed>(seedCap);
		dFrags = st->frags.reserve<Fragment>(winCap);
		dFragFirstSeed = st->fragFirstSeed.reserve<uint32_t>(winCap);
		dJobs = st->jobs.reserve<ReadChainJob>(n);
		GlueRead* dGlueOut = st->glueOut.reserve<GlueRead>(n);
		GlueRead* hGlueOut = st->hGlueOut.reserve<GlueRead>(n);
		jobs = st->hJobs.reserve<ReadChainJob>(n);
		if (H) launchSeedGlueHits(stream, G->dev, R->devOffsets, (uint32_t)n, R->devReadInvalid, H->dev, dSeedOff, dWinCapOff, (uint32_t)P->split_len, (uint32_t)P->split_gap, P->long_pass != 0, stg,
			st->gluePerRead.reserve<uint32_t>(6 * (n + 1)), dPassSeeds, dReadSeeds, dFrags, dFragFirstSeed, dJobs, dGlueOut, dGlueCursors, P->force_global != 0 || clip.on());
		else launchSeedGlue(stream, S->dev, G->dev, R->devOffsets, (uint32_t)n, R->devReadInvalid, dMatches, dReadMatchOff, dReadMatchCount, dSeedOff, dWinCapOff, P->seed_density,
			(uint32_t)P->split_len, (uint32_t)P->split_gap, P->long_pass != 0, stg, st->gluePerRead.reserve<uint32_t>(6 * (n + 1)), dPassSeeds, dReadSeeds, dFrags, dFragFirstSeed, dJobs, dGlueOut, dGlueCursors, P->force_global != 0 || clip.on());
		if (n) HIP_CHECK(hipMemcpyAsync(hGlueOut, dGlueOut, n * sizeof(GlueRead), hipMemcpyDeviceToHost, stream));
		if (n) HIP_CHECK(hipMemcpyAsync(jobs, dJobs, n * sizeof(ReadChainJob), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipMemcpyAsync(hGlueSmall, dGlueCursors, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		syncStream(stream);
		nFrags = hGlueSmall[0]; nSlots = hGlueSmall[1]; traceBudget = hGlueSmall[2];
		maxSlotsPerRead = (uint32_t)std::max<uint64_t>(1, hGlueSmall[3]); maxWindowSeeds = (uint32_t)hGlueSmall[4];
		for (uint64_t r = 0; r < n; r++) {
			ReadGlue& gl = glue[r];
			gl.reset();
			const GlueRead& g = hGlueOut[r];
			gl.failed = g.failed != 0;
			gl.nSeedsR = g.nSeeds; gl.nWindows = g.nFrags;
			gl.seedBegin = g.seedOff; gl.longSeedBegin = g.seedOff;
			gl.fragBegin = g.fragBegin; gl.slotBegin = g.slotBegin;
		}
		// host copies for the result assembly: the fragments always; the seeds only for the seed_* arrays / the anchor traces
		frags = st->hFrags.reserve<Fragment>(nFrags);
		if (nFrags) HIP_CHECK(hipMemcpyAsync(frags, dFrags, nFrags * sizeof(Fragment), hipMemcpyDeviceToHost, stream));
		if (P->keep_seeds || P->keep_traces == 1) {
			readSeeds = st->hReadSeeds.reserve<FragSeed>(seedCap);
			fragFirstSeed = st->hFragFirstSeed.reserve<uint32_t>(nFrags);
			if (seedCap) HIP_CHECK(hipMemcpyAsync(readSeeds, dReadSeeds, seedCap * sizeof(FragSeed), hipMemcpyDeviceToHost, stream));
			if (nFrags) HIP_CHECK(hipMemcpyAsync(fragFirstSeed, dFragFirstSeed, nFrags * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		}
		glueCopied = st->ev[11];
		HIP_CHECK(hipEventRecord(glueCopied, stream));
		tOrdered = nowUs();
	}

