// gc_batch.hip, stage by stage (r6: one file of 2 000 lines before): what comes down: anchors, chains, stitched paths, the chains' NW distances; the pass thread's join.
// Member functions of struct BatchRun - this file is included INSIDE the struct's body (gc_batch.hip), which holds the members, the constructor and run().
	// ---------------- anchors, chains and stitched paths come down (pinned staging)
	void resultsBack()
	{
		// ---------------- results back (pinned staging)
		deviceAnchors = P->keep_traces != 1 && !sw.hostAnchors;   // (GC_HOST_ANCHORS=1: test hook, the host's walk over the slots as before r5)
		anchors = st->hAnchors.reserve<AnchorRec>(deviceAnchors ? 1 : nSlots);
		fragStatus = st->hFragStatus.reserve<uint32_t>(deviceAnchors ? 1 : nFrags);
		fragExtended = st->hFragExtended.reserve<uint32_t>(deviceAnchors ? 1 : nFrags);
		readTies = st->hReadTies.reserve<uint32_t>(n);
		chainOut = st->hChainOut.reserve<uint32_t>(nSlots);
		chainLen = st->hChainLen.reserve<uint32_t>(n);
		chainScore = st->hChainScore.reserve<unsigned long long>(n);
		chainStatus = st->hChainStatus.reserve<uint32_t>(n);
		if (!deviceAnchors) {
			if (nSlots) HIP_CHECK(hipMemcpyAsync(anchors, dAnchors, nSlots * sizeof(AnchorRec), hipMemcpyDeviceToHost, stream));
			if (nFrags) HIP_CHECK(hipMemcpyAsync(fragStatus, dFragStatus, nFrags * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
			if (nFrags) HIP_CHECK(hipMemcpyAsync(fragExtended, dFragExtended, nFrags * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		}
		if (n) HIP_CHECK(hipMemcpyAsync(readTies, dReadTies, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		if (nSlots) HIP_CHECK(hipMemcpyAsync(chainOut, dChainOut, nSlots * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		if (n) HIP_CHECK(hipMemcpyAsync(chainLen, dChainLen, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		if (n) HIP_CHECK(hipMemcpyAsync(chainStatus, dChainStatus, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		if (n) HIP_CHECK(hipMemcpyAsync(chainScore, dChainScore, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipMemcpyAsync(hSmall, dCursors, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipMemcpyAsync(hSmall + 8, dCounters, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		syncStream(stream);
		{
			auto pairUs = [&](int k) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, st->fragEv[2 * k], st->fragEv[2 * k + 1])); return (double)ms * 1000.0; };
			res->kernel_us[1] = res->kernel_us[2] = 0;
			for (uint32_t k = 0; k < nExtendPairs; k++) res->kernel_us[1] += pairUs((int)k);          // k_extend, all rounds (with their retry launches)
			for (uint32_t k = 0; k < nAnchorPairs; k++) res->kernel_us[2] += pairUs(4 + (int)k);      // k_build_anchors, all rounds
		}
		res->kernel_us[3] = elapsedUs(4, 5);
		for (int i = 0; i < 8; i++) res->counters[i] = hSmall[8 + i];
		if (sw.debugTimes) fprintf(stderr, "[gc frag] %llu of %llu fragment extensions handed to the plain-layout kernel\n", hSmall[8 + 6], hSmall[8 + 4]);
#ifdef GC_FRAG_STAMPS
		{
			unsigned long long cyc[8] = { 0 };
			HIP_CHECK(hipMemcpy(cyc, (unsigned long long*)st->fragClaims.ptr + 8, sizeof(cyc), hipMemcpyDeviceToHost));
			fprintf(stderr, "[gc frag stamps] wave-cycles: columns %llu fetch %llu tile_end %llu pop %llu finish %llu walk %llu\n", cyc[0], cyc[1], cyc[2], cyc[3], cyc[4], cyc[5]);
		}
#endif
		// (the cursors overshoot when a pool is full: the extensions / fragments that did not fit carry an overflow status and their reads are flagged)
		uint64_t traceUsed = std::min<uint64_t>(hSmall[1], traceBudget), pathUsed = std::min<uint64_t>(hSmall[2], pathCapacity);
		pathPool = st->hPathPool.reserve<uint32_t>(deviceAnchors ? 1 : pathUsed);
		if (pathUsed && !deviceAnchors) HIP_CHECK(hipMemcpyAsync(pathPool, dPathPool, pathUsed * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		anchorTraces = P->keep_traces == 1;   // (keep_traces == 2: the alignments' traces only - what the output encoders read)
		if (anchorTraces) {
			extResults.resize(nWork);
			tracePool.resize(traceUsed);
			if (nWork) HIP_CHECK(hipMemcpyAsync(extResults.data(), dResults, (size_t)nWork * sizeof(ExtResult), hipMemcpyDeviceToHost, stream));
			if (traceUsed) HIP_CHECK(hipMemcpyAsync(tracePool.data(), dTrace, traceUsed * sizeof(PoolCell), hipMemcpyDeviceToHost, stream));
		}
		syncStream(stream);
		res->host_us[3] = nowUs() - tDev;   // K3..K4 + their transfers, wall
		// the stitched node paths come down behind the kernels that follow on this stream; they are only needed for the result arrays
		if (deviceStitch) {
			uint64_t used = std::min<uint64_t>(*hStitchCursor, stitchDenseCap);
			hStitchNodes = st->hStitchNodes.reserve<uint32_t>(std::max<uint64_t>(1, used));
			if (used) HIP_CHECK(hipMemcpyAsync(hStitchNodes, dStitchNodes, used * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
			stitchNodesPending = true;
		}

	}

	// ---------------- r5: the anchors the reference keeps of every read as the result's dense arrays, made on the device (gc_results.hip)
	void compactAnchors()
	{
		if (!deviceAnchors) return;
		uint4* dPerRead = st->anchorPerRead.reserve<uint4>(n);
		uint32_t* dSlotEnd = st->anchorSlotEnd.reserve<uint32_t>(n);
		unsigned long long* dOff = st->anchorOff.reserve<unsigned long long>(2 * n + 2);
		hAnchorPerRead = st->hAnchorPerRead.reserve<uint4>(n);
		hAnchorOff = st->hAnchorOff.reserve<unsigned long long>(2 * n + 4);
		unsigned long long* hTotals = hAnchorOff + 2 * n + 2;
		hTotals[0] = hTotals[1] = 0;
		launchAnchorCounts(stream, dJobs, (uint32_t)n, dFrags, dFragStatus, dFragExtended, dAnchors, dPerRead, dSlotEnd, dOff, hTotals);
		if (n) HIP_CHECK(hipMemcpyAsync(hAnchorPerRead, dPerRead, n * sizeof(uint4), hipMemcpyDeviceToHost, stream));
		if (n) HIP_CHECK(hipMemcpyAsync(hAnchorOff, dOff, (2 * n + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
		syncStream(stream);
		denseAnchors = n ? hAnchorOff[2 * n] : 0; densePathWords = n ? hAnchorOff[2 * n + 1] : 0;
		// one block for the eleven arrays: nine of 4 bytes per anchor, the 8-byte path offsets, the path words
		const uint64_t A = denseAnchors, bytes = A * 44 + densePathWords * 4 + 64;
		uint8_t* dDense = st->anchorDense.reserve<uint8_t>(bytes);
		hAnchorDense = st->hAnchorDense.reserve<uint8_t>(bytes);
		AnchorArrays out;
		out.pathOff = (unsigned long long*)dDense;
		uint32_t* w = (uint32_t*)(dDense + 8 * A);
		out.x = w; out.y = w + A; out.firstNode = w + 2 * A; out.firstOffset = w + 3 * A; out.firstSeqPos = w + 4 * A; out.lastNode = w + 5 * A; out.lastOffset = w + 6 * A; out.lastSeqPos = w + 7 * A;
		out.score = (int32_t*)(w + 8 * A); out.path = w + 9 * A;
		launchAnchorCompact(stream, dJobs, (uint32_t)n, dAnchors, dPathPool, dSlotEnd, dOff, out);
		if (A) HIP_CHECK(hipMemcpyAsync(hAnchorDense, dDense, A * 44 + densePathWords * 4, hipMemcpyDeviceToHost, stream));
		syncStream(stream);
	}
	// the dense arrays in the staging block (the layout compactAnchors gave the device's)
	const unsigned long long* densePathOff() const { return (const unsigned long long*)hAnchorDense; }
	const uint32_t* denseWords(int k) const { return (const uint32_t*)(hAnchorDense + 8 * denseAnchors) + (uint64_t)k * denseAnchors; }   // 0 x, 1 y, 2-4 first node / offset / seqPos, 5-7 last, 8 score, 9 the path words

	// ---------------- gc_params::fast_mode: x of the chain's first anchor and y of its last (src/Aligner.cpp:836; the chain's, whichever piece of it is the longest)
	void chainSpan(uint64_t r, uint32_t& x, uint32_t& y) const
	{
		const uint32_t* ids = chainOut + jobs[r].chainBegin;
		const uint32_t first = ids[0], last = ids[chainLen[r] - 1];
		if (deviceAnchors) {   // chain index = index among the read's dense anchors
			const uint64_t a0 = hAnchorOff[2 * r];
			x = denseWords(0)[a0 + first]; y = denseWords(1)[a0 + last];
			return;
		}
		const ReadGlue& gl = glue[r];   // ... = index among the anchors the walk over the read's slots keeps
		uint64_t slot = gl.slotBegin;
		uint32_t kept = 0;
		for (size_t f = 0; f < gl.nWindows; f++) {
			const uint64_t F = gl.fragBegin + f;
			const uint32_t nS = frags[F].seedEnd - frags[F].seedBegin;
			if (fragStatus[F] == 1) break;
			for (uint32_t k = 0; k < nS; k++) if (anchors[slot + k].valid) {
				if (kept == first) x = anchors[slot + k].x;
				if (kept == last) y = anchors[slot + k].y;
				kept++;
			}
			slot += nS;
		}
	}

	// ---------------- host stitching of what the kernel declined; NW distance of every stitched path against its read
	void stitchAndChainDistances()
	{
		// ---------------- chain stitching (src/Aligner.cpp:754-822) on the host workers, while the whole-read pass still runs
		double tStitch = nowUs();
		std::atomic<uint64_t> hostStitched { 0 };
		if (P->stitch) {
			pool.run(n, [&](size_t r, size_t) {
				ReadGlue& gl = glue[r];
				gl.stitchedOnDevice = false;
				if (chainStatus[r] != 0 || chainLen[r] == 0) return;
				if (deviceStitch && stitchInfo[r].status == 0) {
					const StitchInfo& si = stitchInfo[r];
					gl.stitched.nodes.clear();   // filled once the download has finished (below)
					gl.stitched.firstOffset = si.firstOffset; gl.stitched.lastOffset = si.lastOffset; gl.stitched.cells = si.cells;
					gl.stitchedOnDevice = true;
					return;
				}
				hostStitched++;
				if (deviceStitch && sw.debugTimes) fprintf(stderr, "[gc stitch] read %zu goes to the host: reason %u, chain of %u anchors\n", r, stitchInfo[r].status, chainLen[r]);
				std::vector<uint32_t> slots;
				if (deviceAnchors) {   // the read's kept anchors are the dense arrays' [a0, a1): chain index = dense index
					const uint64_t a0 = hAnchorOff[2 * r], a1 = hAnchorOff[2 * r + 2];
					std::vector<AnchorRec> recs(a1 - a0);
					slots.resize(a1 - a0);
					for (uint64_t a = a0; a < a1; a++) {
						AnchorRec& rec = recs[a - a0];
						rec.valid = 1; rec.x = denseWords(0)[a]; rec.y = denseWords(1)[a];
						rec.firstNode = denseWords(2)[a]; rec.firstOffset = denseWords(3)[a]; rec.firstSeqPos = denseWords(4)[a] - rec.x;
						rec.lastNode = denseWords(5)[a]; rec.lastOffset = denseWords(6)[a]; rec.lastSeqPos = denseWords(7)[a] - rec.x;
						rec.score = (int32_t)denseWords(8)[a];
						rec.pathOff = densePathOff()[a];
						rec.pathLen = (uint32_t)((a + 1 < denseAnchors ? densePathOff()[a + 1] : densePathWords) - densePathOff()[a]);
						rec.pad = 0;
						slots[a - a0] = (uint32_t)(a - a0);
					}
					stitchChain(hg, (long long)P->colinear_gap, chainOut + jobs[r].chainBegin, chainLen[r], slots.data(), recs.data(), denseWords(9), gl.stitched);
					return;
				}
				uint64_t slot = gl.slotBegin;
				for (size_t f = 0; f < gl.nWindows; f++) {
					uint64_t F = gl.fragBegin + f;
					uint32_t nS = frags[F].seedEnd - frags[F].seedBegin;
					if (fragStatus[F] == 1) break;   // `cont` is never reset (src/Aligner.cpp:695-703)
					for (uint32_t k = 0; k < nS; k++) if (anchors[slot + k].valid) slots.push_back((uint32_t)(slot + k - gl.slotBegin));
					slot += nS;
				}
				stitchChain(hg, (long long)P->colinear_gap, chainOut + jobs[r].chainBegin, chainLen[r], slots.data(), anchors + gl.slotBegin, pathPool, gl.stitched);
			});
		}
		// ---------------- edit distance of the stitched path against the read (edlibAlign at src/Aligner.cpp:845, value only):
		// path letters are spelled out on the device from the node path, then the NW kernel; still behind the whole-read pass
		std::function<void()> finishChainEditDistances;
		std::vector<uint32_t> pairRead;   // chain pairs -> read
		if (P->stitch && P->edit_distances) {
			uint64_t nNodesTotal = 0, nCells = 0;
			uint32_t nPairs = 0;
			// node paths stitched on the device are read where k_stitch left them; only the ones stitched here go up
			for (uint64_t r = 0; r < n; r++) { glue[r].stitchedBegin = nNodesTotal; if (!glue[r].stitchedOnDevice) nNodesTotal += glue[r].stitched.nodes.size(); }
			uint32_t* hNodes = st->hEdPathNodes.reserve<uint32_t>(nNodesTotal);
			PathSeqJob* hJobsPS = st->hEdJobs.reserve<PathSeqJob>(n);
			EdPair* hPairs = st->hEdPairs.reserve<EdPair>(n);
			int64_t* hOut = st->hEdOut.reserve<int64_t>(n);
			for (uint64_t r = 0; r < n; r++) {
				const StitchedPath& sp = glue[r].stitched;
				const bool onDevice = glue[r].stitchedOnDevice;
				if (!onDevice && !sp.nodes.empty()) memcpy(hNodes + glue[r].stitchedBegin, sp.nodes.data(), sp.nodes.size() * sizeof(uint32_t));
				if (sp.cells >= 0x7fffffffull) throw std::runtime_error("stitched path too long");
				hJobsPS[r] = PathSeqJob { onDevice ? stitchInfo[r].start : ((1ull << 63) | glue[r].stitchedBegin), nCells, onDevice ? stitchInfo[r].len : (uint32_t)sp.nodes.size(), (uint32_t)sp.cells, sp.firstOffset, sp.lastOffset };
				if (sp.cells && !P->fast_mode) {
					uint32_t len = (uint32_t)(R->offsets[r + 1] - R->offsets[r]);
					// first band: the length difference plus ~14 % of the shorter sequence (ONT-like error rates pass in one sweep) - widened to 20 %
					// where that still fits the two-pairs-per-wave kernel: a wave's time follows the number of columns, not the band, so the wider
					// band is free there and spares the pairs above 14 % their second sweep
					uint32_t cells = (uint32_t)sp.cells, shorter = std::min(cells, len), longer = std::max(cells, len);
					uint32_t firstBand = (longer - shorter) + std::max<uint32_t>(64, shorter / 7);
					const uint32_t halfLimit = editDistanceMaxK(0);
					if (firstBand < halfLimit) firstBand = std::max(firstBand, std::min<uint32_t>(halfLimit - 1, (longer - shorter) + shorter / 5));
					// three pairs per wave where the length difference plus 10 % of the shorter sequence fit the band a team of 21 lanes holds (launchEditDistances widens the band to all of it):
					// with column groups that band is 1 441, and cfg2's chain pairs (distances 1 100-1 300) pass it in one sweep
					const uint32_t thirdLimit = editDistanceTeamMaxK(3);
					if (len <= 65536 && (longer - shorter) + shorter / 10 < thirdLimit) firstBand = thirdLimit - 1;
					hPairs[nPairs++] = EdPair { nCells, cells, (uint32_t)r, (uint32_t)r, firstBand };
					pairRead.push_back((uint32_t)r);
				}
				nCells += sp.cells;
			}
			uint32_t* dNodes = st->edPathNodes.reserve<uint32_t>(nNodesTotal);
			PathSeqJob* dJobsPS = st->edJobs.reserve<PathSeqJob>(n);
			char* dLetters = st->edLetters.reserve<char>(nCells);
			uint32_t* dLettersLen = st->edLettersLen.reserve<uint32_t>(n);
			EdPair* dPairs = st->edPairs.reserve<EdPair>(n);
			int64_t* dOut = st->edOut.reserve<int64_t>(n);
			if (nNodesTotal) HIP_CHECK(hipMemcpyAsync(dNodes, hNodes, nNodesTotal * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
			if (n) HIP_CHECK(hipMemcpyAsync(dJobsPS, hJobsPS, n * sizeof(PathSeqJob), hipMemcpyHostToDevice, stream));
			launchChainPathSeq(stream, G->dev, dJobsPS, (uint32_t)n, dStitchNodes, dNodes, dLetters, dLettersLen);
			chainLetterJobs = hJobsPS;
			dChainLetters = dLetters;
			dChainAltNodes = dNodes;
			if (P->fast_mode) {
				// gc_params::fast_mode (src/Aligner.cpp:834-843): no NW distance of the chain. The score is the number of stitched cells whose letter is not the read's at
				// min(y, x + j), counted by k_fast_chain_score from the letters just spelled; the pairs are not handed to launchEditDistances
				FastChainJob* hJobsF = st->hFastJobs.reserve<FastChainJob>(n);
				int64_t* hScore = st->hFastScore.reserve<int64_t>(n);
				uint64_t nFast = 0;
				for (uint64_t r = 0; r < n; r++) {
					const PathSeqJob& pj = hJobsPS[r];
					FastChainJob job { pj.srcOff, pj.outOff, R->offsets[r], 0, pj.count, pj.outCap, pj.firstOffset, pj.lastOffset, 0, 0 };
					if (job.cells) {
						chainSpan(r, job.x, job.y);
						if (job.y >= R->offsets[r + 1] - R->offsets[r]) throw std::runtime_error("internal: a chain's last anchor ends beyond its read");   // (y = l + len - 1, :707)
						nFast++;
					}
					hJobsF[r] = job;
				}
				FastChainJob* dJobsF = st->fastJobs.reserve<FastChainJob>(n);
				int64_t* dScore = st->fastScore.reserve<int64_t>(n);
				hipEvent_t timed[2] = { nullptr, nullptr };
				if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
				if (n) HIP_CHECK(hipMemcpyAsync(dJobsF, hJobsF, n * sizeof(FastChainJob), hipMemcpyHostToDevice, stream));
				if (timed[0]) HIP_CHECK(hipEventRecord(timed[0], stream));
				launchFastChainScore(stream, dJobsF, (uint32_t)n, dLetters, dLettersLen, R->devBases, dScore);
				if (timed[1]) HIP_CHECK(hipEventRecord(timed[1], stream));
				if (n) HIP_CHECK(hipMemcpyAsync(hScore, dScore, n * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
				fastChainJobs = hJobsF;
				finishChainEditDistances = [=]() {   // only collects the counts
					syncStream(stream);
					for (uint64_t r = 0; r < n; r++) {
						if (!hJobsF[r].cells) continue;
						ReadGlue& gl = glue[r];
						gl.chainEditDistance = hScore[r];
						if (hScore[r] < 0) { gl.chainEditDistance = -1; gl.capacityExceeded = true; }
					}
					if (timed[0]) {
						float ms = 0;
						HIP_CHECK(hipEventElapsedTime(&ms, timed[0], timed[1]));
						for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
						fprintf(stderr, "[gc times] fast mode: k_fast_chain_score over %llu stitched reads, %llu cells, %.3f ms on the device; no k_edit_distance launch for the chains\n", (unsigned long long)nFast, (unsigned long long)nCells, ms);
					}
				};
			} else {
				auto readLenOf = [R = R](uint32_t r) { return (uint32_t)(R->offsets[r + 1] - R->offsets[r]); };
				launchEditDistances(st->edChainRun, stream, hPairs, hOut, nPairs, dPairs, dOut, R->devEdReads, R->devBases, R->devEqMasks, dLetters, dLettersLen, readLenOf, sw.debugTimes);
				finishChainEditDistances = [=, &pairRead]() {   // waits for the kernels (they run beside the whole-read pass) and reruns the few pairs that need a wider band
					finishEditDistances(st->edChainRun, stream, hPairs, hOut, nPairs, dPairs, dOut, R->devEdReads, R->devBases, R->devEqMasks, dLetters, dLettersLen, sw.debugTimes);
					if (sw.debugEd) for (uint32_t i = 0; i < nPairs && i < 400; i++) {
						const uint32_t r = pairRead[i];
						fprintf(stderr, "[gc ed] read %u len %llu path %llu chain %u scoreSum %u onDevice %d distance %lld\n", r, (unsigned long long)(R->offsets[r + 1] - R->offsets[r]), (unsigned long long)glue[r].stitched.cells,
							chainLen[r], deviceStitch ? stitchInfo[r].scoreSum : 0u, (int)glue[r].stitchedOnDevice, (long long)hOut[i]);
					}
					for (uint32_t i = 0; i < nPairs; i++) {
						ReadGlue& gl = glue[pairRead[i]];
						gl.chainEditDistance = hOut[i];
						if (hOut[i] < -1) { gl.chainEditDistance = -1; gl.capacityExceeded = true; }
					}
				};
			}
		}
		if (finishChainEditDistances) finishChainEditDistances();   // this thread would only wait for the whole-read pass otherwise
		if (stitchNodesPending) {
			syncStream(stream);
			pool.run(n, [&](size_t r, size_t) {
				if (!glue[r].stitchedOnDevice) return;
				const StitchInfo& si = stitchInfo[r];
				glue[r].stitched.nodes.assign(hStitchNodes + si.start, hStitchNodes + si.start + si.len);
			});
		}
		double stitchUs = nowUs() - tStitch;
		if (sw.debugTimes) fprintf(stderr, "[gc cpu] %.0f ms up to the end of stitching + chain edit distances\n", processCpuMs() - cpuCall);
		if (sw.debugTimes) fprintf(stderr, "[gc times] chain stitching + its edit distances %.1f ms (%llu reads stitched on the host)\n", stitchUs / 1e3, (unsigned long long)hostStitched.load());
		res->counters[7] = hostStitched.load();   // reads whose chain was stitched on the host

	}

	// ---------------- gc_params::colinear_chaining == 0 (--no-colinear-chaining, src/Aligner.cpp:596-600): the fragment extension, anchors, chaining, stitching and the chain's
	// NW distance are neither launched nor allocated; the result assembly reads all-zero per-read records in their place, so every such array comes back empty
	void withoutChaining()
	{
		zeroWords.assign(n + 1, 0); zeroLongs.assign(2 * n + 4, 0); zeroPerRead.assign(n + 1, make_uint4(0, 0, 0, 0));
		deviceAnchors = true; anchorTraces = P->keep_traces == 1;   // (the result keeps its one-entry anchor_trace_off)
		hAnchorPerRead = zeroPerRead.data(); hAnchorOff = zeroLongs.data();
		denseAnchors = densePathWords = 0;
		readTies = chainLen = chainStatus = zeroWords.data();
		chainScore = zeroLongs.data();
	}


