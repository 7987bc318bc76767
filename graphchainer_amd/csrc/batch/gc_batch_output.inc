// gc_batch.hip, stage by stage (r6: one file of 2 000 lines before): the chained alignments' traces and the flat result. The output encoders on the device, which run
// between the two, are a class of their own (OutputEncoder, batch/gc_output_encoder.hpp): assemble() hands it the result to fill.
// Member functions of struct BatchRun - this file is included INSIDE the struct's body (gc_batch.hip), which holds the members, the constructor and run().
	// ---------------- edlib path + trace of the chained alignments that are wanted (src/Aligner.cpp:845-905)
	void chainedAlignments()
	{
		// ---------------- the chained alignment (src/Aligner.cpp:845-905): edlib's alignment path of (stitched path, read) from k_edit_path,
		// walked over the path cells and the read into the trace; then the decision. Only reads whose chained alignment can still win
		// (or all with chain_traces == 2) are traced: the path does not change the edit distance that decides.
		double tChainTrace = nowUs();
		uint64_t nChainTraced = 0;
		if (fastChainJobs) { nChainTraced = fastChainedAlignments(); }
		else if (P->stitch && P->edit_distances && chainLetterJobs) {
			auto beats = [&](const ReadGlue& gl) { return gl.longSelected.empty() || gl.longEditDistance > gl.chainEditDistance; };   // :905
			std::vector<uint32_t> cand;
			for (uint64_t r = 0; r < n; r++) {
				const ReadGlue& gl = glue[r];
				if (gl.longFailed || gl.stitched.cells == 0 || gl.chainEditDistance < 0) continue;
				if (P->chain_traces >= 2 || (P->chain_traces == 1 && beats(gl))) cand.push_back((uint32_t)r);
			}
			nChainTraced = cand.size();
			if (!cand.empty()) {
				const size_t m = cand.size();
				EdPathJob* hJobsEP = st->hEdPathJobs.reserve<EdPathJob>(m);
				uint64_t opsTotal = 0;
				uint32_t maxQ = 1, maxT = 1;
				for (size_t i = 0; i < m; i++) {
					const uint32_t r = cand[i];
					const uint32_t q = (uint32_t)glue[r].stitched.cells, t = (uint32_t)(R->offsets[r + 1] - R->offsets[r]);
					hJobsEP[i] = EdPathJob { chainLetterJobs[r].outOff, R->offsets[r], opsTotal, q, t, (int32_t)glue[r].chainEditDistance, 0 };
					opsTotal += (uint64_t)q + t;
					maxQ = std::max(maxQ, q); maxT = std::max(maxT, t);
				}
				EdPathJob* dJobsEP = st->edPathJobs.reserve<EdPathJob>(m);
				uint8_t* dOps = st->edPathOps.reserve<uint8_t>(opsTotal);
				uint32_t* dOpsLen = st->edPathLen.reserve<uint32_t>(m);
				uint8_t* dScratchEP = st->edPathScratch.reserve<uint8_t>((uint64_t)editPathGridBlocks((uint32_t)m) * editPathScratchBytes(maxQ, maxT));
				uint8_t* hOps = st->hEdPathOps.reserve<uint8_t>(opsTotal);
				uint32_t* hOpsLen = st->hEdPathLen.reserve<uint32_t>(m);
				HIP_CHECK(hipMemcpyAsync(dJobsEP, hJobsEP, m * sizeof(EdPathJob), hipMemcpyHostToDevice, stream));
				launchEditPath(stream, dJobsEP, (uint32_t)m, dChainLetters, R->devBases, dScratchEP, maxQ, maxT, dOps, dOpsLen);
				HIP_CHECK(hipMemcpyAsync(hOpsLen, dOpsLen, m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
				HIP_CHECK(hipMemcpyAsync(hOps, dOps, opsTotal, hipMemcpyDeviceToHost, stream));
				syncStream(stream);
				pool.run(m, [&](size_t i, size_t) {
					const uint32_t r = cand[i];
					ReadGlue& gl = glue[r];
					const uint64_t readLen = R->offsets[r + 1] - R->offsets[r];
					// `longest`: one (node, offset) per base of the stitched piece (pathToTrace, src/Aligner.cpp:409-424)
					std::vector<std::pair<uint32_t, uint32_t>> cells;
					cells.reserve(gl.stitched.cells);
					for (uint32_t node : gl.stitched.nodes) {
						uint32_t S = 0, L = (uint32_t)hg.NodeLength(node);
						if (node == gl.stitched.nodes[0]) S = gl.stitched.firstOffset;
						else if (node == gl.stitched.nodes.back()) L = gl.stitched.lastOffset + 1;
						for (uint32_t o = S; o < L; o++) cells.emplace_back(node, o);
					}
					const uint8_t* ops = hOps + hJobsEP[i].opsOff;
					const uint32_t nOps = hOpsLen[i];
					if (cells.empty() || nOps == 0) return;   // no alignment from edlib: no chained alignment item (:890)
					// :848-876: one trace cell per op, recorded before the op advances; indices clamped to the last cell / base
					uint64_t pos_i = 0, seq_i = 0;
					gl.chainTraceNode.resize(nOps); gl.chainTraceOffset.resize(nOps); gl.chainTraceSeqPos.resize(nOps); gl.chainTraceSwitch.assign(nOps, 0);
					uint32_t prevSplit = 0;
					for (uint32_t j = 0; j < nOps; j++) {
						const uint32_t node = cells[pos_i].first, off = cells[pos_i].second;
						gl.chainTraceNode[j] = hg.nodeIDs[node];                       // :886-887 output coordinates
						gl.chainTraceOffset[j] = (uint32_t)(off + hg.nodeOffset[node]);
						gl.chainTraceSeqPos[j] = (uint32_t)seq_i;
						if (j > 0 && node != prevSplit) gl.chainTraceSwitch[j - 1] = 1;      // :880-882 (split nodes compared)
						prevSplit = node;
						const uint8_t c = ops[j];
						if (c == 0 || c == 3) { pos_i++; seq_i++; }
						else if (c == 1) pos_i++;
						else if (c == 2) seq_i++;
						seq_i = std::min<uint64_t>(seq_i, readLen - 1);
						pos_i = std::min<uint64_t>(pos_i, cells.size() - 1);
					}
					gl.chainAlnStart = gl.chainTraceSeqPos[0];
					gl.chainAlnEnd = gl.chainTraceSeqPos[nOps - 1] + 1;
					// :904 SelectAlignments(method All) still applies --E-cutoff; :905 the decision
					gl.hasChainAlignment = evalueModel.keeps(P->e_cutoff, hg.SizeInBP(), readLen, gl.chainAlnEnd - gl.chainAlnStart, (size_t)gl.chainEditDistance);
					if (!gl.hasChainAlignment) { gl.chainTraceNode.clear(); gl.chainTraceOffset.clear(); gl.chainTraceSeqPos.clear(); gl.chainTraceSwitch.clear(); gl.chainAlnStart = gl.chainAlnEnd = 0; }
					gl.chainWins = gl.hasChainAlignment && beats(gl);
				});
			}
			if (P->chain_traces == 0) {
				// no traces asked for: the decision from the distances alone (an alignment edlib cannot build or --E-cutoff drops would differ)
				for (uint64_t r = 0; r < n; r++) { ReadGlue& gl = glue[r]; gl.chainWins = !gl.longFailed && gl.stitched.cells > 0 && gl.chainEditDistance >= 0 && beats(gl); }
			}
		}
		if (sw.debugTimes) fprintf(stderr, "[gc times] chained alignment traces: %llu reads, %.1f ms\n", (unsigned long long)nChainTraced, (nowUs() - tChainTrace) / 1e3);

	}

	// ---------------- gc_params::fast_mode (src/Aligner.cpp:834-843,880-905): the chained alignment is the stitched piece itself, cell j at read position min(y, x + j). Its score
	// (k_fast_chain_score's count) and its bounds are known without the trace, so --E-cutoff (:904) and the decision (:905) come first, for every stitched read in every
	// chain_traces mode; k_fast_chain_trace then writes the cells of the reads whose trace is wanted (1: the winners, 2: every read with a chained alignment) in place of
	// k_edit_path and the host's walk over edlib's ops. Returns the number of reads traced.
	uint64_t fastChainedAlignments()
	{
		std::vector<uint32_t> cand;
		uint64_t cellsTotal = 0;
		for (uint64_t r = 0; r < n; r++) {
			ReadGlue& gl = glue[r];
			const FastChainJob& job = fastChainJobs[r];
			if (gl.longFailed || job.cells == 0 || gl.chainEditDistance < 0) continue;
			const uint64_t readLen = R->offsets[r + 1] - R->offsets[r];
			const uint32_t alnStart = job.x, alnEnd = std::min<uint64_t>(job.y, (uint64_t)job.x + job.cells - 1) + 1;   // :894-895 of the trace below
			gl.hasChainAlignment = evalueModel.keeps(P->e_cutoff, hg.SizeInBP(), readLen, alnEnd - alnStart, (size_t)gl.chainEditDistance);
			gl.chainWins = gl.hasChainAlignment && (gl.longSelected.empty() || gl.longEditDistance > gl.chainEditDistance);
			if (!gl.hasChainAlignment || !(P->chain_traces >= 2 || (P->chain_traces == 1 && gl.chainWins))) continue;
			gl.chainAlnStart = alnStart; gl.chainAlnEnd = alnEnd;   // (reported with the trace, as in the default mode)
			cand.push_back((uint32_t)r);
			cellsTotal += job.cells;
		}
		const size_t m = cand.size();
		if (m == 0) return 0;
		FastChainJob* hJobsT = st->hFastTraceJobs.reserve<FastChainJob>(m);
		uint64_t at = 0;
		for (size_t i = 0; i < m; i++) { hJobsT[i] = fastChainJobs[cand[i]]; hJobsT[i].traceOff = at; at += hJobsT[i].cells; }
		// one block laid out like the result's four arrays: node ids, offsets, read positions (4 bytes a cell each), switches (1 byte)
		const uint64_t T = cellsTotal, bytes = 13 * T;
		FastChainJob* dJobsT = st->fastTraceJobs.reserve<FastChainJob>(m);
		uint8_t* dTraceBlock = st->fastTrace.reserve<uint8_t>(bytes);
		uint32_t* dWritten = st->fastWritten.reserve<uint32_t>(m);
		uint8_t* hTraceBlock = st->hFastTrace.reserve<uint8_t>(bytes);
		uint32_t* hWritten = st->hFastWritten.reserve<uint32_t>(m);
		hipEvent_t timed[2] = { nullptr, nullptr };
		if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
		HIP_CHECK(hipMemcpyAsync(dJobsT, hJobsT, m * sizeof(FastChainJob), hipMemcpyHostToDevice, stream));
		if (timed[0]) HIP_CHECK(hipEventRecord(timed[0], stream));
		launchFastChainTrace(stream, G->dev, dJobsT, (uint32_t)m, dStitchNodes, dChainAltNodes, (int32_t*)dTraceBlock, (uint32_t*)(dTraceBlock + 4 * T), (uint32_t*)(dTraceBlock + 8 * T), dTraceBlock + 12 * T, dWritten);
		if (timed[1]) HIP_CHECK(hipEventRecord(timed[1], stream));
		HIP_CHECK(hipMemcpyAsync(hWritten, dWritten, m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipMemcpyAsync(hTraceBlock, dTraceBlock, bytes, hipMemcpyDeviceToHost, stream));
		syncStream(stream);
		if (timed[0]) {
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, timed[0], timed[1]));
			for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
			fprintf(stderr, "[gc times] fast mode: k_fast_chain_trace over %zu reads, %llu cells, %.3f ms on the device; no k_edit_path launch\n", m, (unsigned long long)T, ms);
		}
		for (size_t i = 0; i < m; i++) if (hWritten[i] != hJobsT[i].cells) throw std::runtime_error("internal: the fast-mode trace kernel and the stitched path disagree on a read's cell count");
		const int32_t* tNode = (const int32_t*)hTraceBlock; const uint32_t* tOffset = (const uint32_t*)(hTraceBlock + 4 * T); const uint32_t* tSeqPos = (const uint32_t*)(hTraceBlock + 8 * T);
		const uint8_t* tSwitch = hTraceBlock + 12 * T;
		pool.run(m, [&](size_t i, size_t) {
			ReadGlue& gl = glue[cand[i]];
			const uint64_t b = hJobsT[i].traceOff, e = b + hJobsT[i].cells;
			gl.chainTraceNode.assign(tNode + b, tNode + e); gl.chainTraceOffset.assign(tOffset + b, tOffset + e);
			gl.chainTraceSeqPos.assign(tSeqPos + b, tSeqPos + e); gl.chainTraceSwitch.assign(tSwitch + b, tSwitch + e);
		});
		return m;
	}

	// ---------------- the flat result: count per read, prefix-sum, fill in parallel
	void assemble()
	{
		// ---------------- assemble the flat result: count per read, prefix-sum, fill in parallel
		double tAsm = nowUs();
		if (glueCopied) HIP_CHECK(hipEventSynchronize(glueCopied));   // (long since done: the copies were queued before the fragment pipeline)
		std::vector<uint8_t> failedAssertion(n, 0);
		std::vector<uint64_t> seedsExtended(n, 0), seedsExtendedLong(n, 0);
		// read position of the seed in a fragment-pass slot (the device holds the per-slot records; the host keeps seeds and windows)
		auto slotSeqPos = [&](uint64_t r, uint64_t slot, uint64_t F) -> uint32_t {
			(void)r;
			return readSeeds[fragFirstSeed[F] + (slot - frags[F].seedBegin)].seqPos;   // (host copies: kept whenever keep_traces asks for this)
		};
		auto forEachAnchor = [&](uint64_t r, auto&& visit) {   // visit(slotIndex, fragmentIndex) for every anchor the reference would keep
			const ReadGlue& gl = glue[r];
			if (gl.longFailed) return;   // `cont` was already set by the whole-read pass (src/Aligner.cpp:529,591,702)
			uint64_t slot = gl.slotBegin;
			for (size_t f = 0; f < gl.nWindows; f++) {
				uint64_t F = gl.fragBegin + f;
				uint32_t nS = frags[F].seedEnd - frags[F].seedBegin;
				if (fragStatus[F] == 1) return;   // `cont` is never reset: later fragments add nothing (src/Aligner.cpp:695-703)
				for (uint32_t k = 0; k < nS; k++) if (anchors[slot + k].valid) visit(slot + k, F);
				slot += nS;
			}
		};
		pool.run(n, [&](size_t r, size_t) {
			ReadGlue& gl = glue[r];
			failedAssertion[r] = gl.failed ? 1 : 0;
			if (gl.longFailed) {   // the fragment pipeline ran beside the whole-read pass; what it found for this read is dropped
				failedAssertion[r] = 1;
				chainLen[r] = 0; chainScore[r] = 0; chainStatus[r] = 0;
				gl.stitched = StitchedPath();
				gl.chainEditDistance = -1;
				if (P->long_pass) seedsExtendedLong[r] = pass.results()[r].seedsExtended;
				return;
			}
			if (chainStatus[r] != 0) { gl.capacityExceeded = true; chainLen[r] = 0; chainScore[r] = 0; }
			if (deviceAnchors) {   // k_anchor_counts walked the read's fragments and slots
				const uint4 pr = hAnchorPerRead[r];
				if (pr.w & 2u) gl.capacityExceeded = true;
				if (pr.w & 1u) failedAssertion[r] = 1;
				seedsExtended[r] += pr.z;
				gl.nAnchors = pr.x; gl.nPath = pr.y;
			} else
			for (size_t f = 0; f < gl.nWindows; f++) {
				uint64_t F = gl.fragBegin + f;
				if (fragStatus[F] == 2) gl.capacityExceeded = true;   // an extension or the anchor path pool overflowed even in the retry: this fragment gave no anchors
				if (fragStatus[F] == 1) { failedAssertion[r] = 1; break; }
				seedsExtended[r] += fragExtended[F];
			}
			if (P->long_pass) {
				seedsExtendedLong[r] = pass.results()[r].seedsExtended;
				if (pass.results()[r].status == 1) failedAssertion[r] = 1;
			}
			if (!deviceAnchors) forEachAnchor(r, [&](uint64_t slot, uint64_t F) {
				gl.nAnchors++;
				gl.nPath += anchors[slot].pathLen;
				if (anchorTraces) {
					const ExtResult& eb = extResults[2 * slot];
					const ExtResult& ef = extResults[2 * slot + 1];
					uint32_t p = slotSeqPos(r, slot, F) - (anchors[slot].x);
					bool hasB = p > 0 && eb.status == EXT_OK, hasF = p < (uint32_t)P->split_len - 1 && ef.status == EXT_OK;
					gl.nTrace += (hasB ? (hasF ? eb.traceLen - 1 : eb.traceLen) : 0) + (hasF ? ef.traceLen : 0);
				}
			});
		});
		uint64_t nAnchors = 0, nPath = 0, nTrace = 0, nChain = 0, nLong = 0, nLongTrace = 0, nStitched = 0, nLongSelected = 0, nChainTrace = 0;
		for (uint64_t r = 0; r < n; r++) {
			glue[r].anchorBegin = nAnchors; glue[r].pathBegin = nPath; glue[r].traceBegin = nTrace; glue[r].chainBegin = nChain;
			glue[r].longBegin = nLong; glue[r].longTraceBegin = nLongTrace;
			nAnchors += glue[r].nAnchors; nPath += glue[r].nPath; nTrace += glue[r].nTrace; nChain += chainLen[r];
			nLong += glue[r].longAlns.size();
			glue[r].stitchedBegin = nStitched; nStitched += glue[r].stitched.nodes.size();
			glue[r].longSelectedBegin = nLongSelected; nLongSelected += glue[r].longSelected.size();
			glue[r].chainTraceBegin = nChainTrace; nChainTrace += glue[r].chainTraceNode.size();
			if (P->keep_traces) for (const LongAln& a : glue[r].longAlns) nLongTrace += a.traceLen;
		}
		const bool keepSeeds = P->keep_seeds != 0;
		std::vector<uint64_t> seedOutBegin(n + 1, 0);   // the result's seed lists are dense (the device's sit at capacity offsets)
		for (uint64_t r = 0; r < n; r++) seedOutBegin[r + 1] = seedOutBegin[r] + (keepSeeds ? glue[r].nSeedsR : 0);
		const uint64_t nSeedsOut = seedOutBegin[n];
		res->read_seed_off = resultArray<uint64_t>(n + 1);
		res->seed_node = resultArray<uint32_t>(nSeedsOut); res->seed_offset = resultArray<uint32_t>(nSeedsOut);
		res->seed_seqpos = resultArray<uint32_t>(nSeedsOut); res->seed_goodness = resultArray<uint64_t>(nSeedsOut);
		res->read_anchor_off = resultArray<uint64_t>(n + 1);
		res->anchor_x = resultArray<uint32_t>(nAnchors); res->anchor_y = resultArray<uint32_t>(nAnchors);
		res->anchor_path_off = resultArray<uint64_t>(nAnchors + 1); res->anchor_path = resultArray<uint32_t>(nPath);
		res->anchor_first_node = resultArray<uint32_t>(nAnchors); res->anchor_first_offset = resultArray<uint32_t>(nAnchors); res->anchor_first_seqpos = resultArray<uint32_t>(nAnchors);
		res->anchor_last_node = resultArray<uint32_t>(nAnchors); res->anchor_last_offset = resultArray<uint32_t>(nAnchors); res->anchor_last_seqpos = resultArray<uint32_t>(nAnchors);
		res->anchor_score = resultArray<int32_t>(nAnchors);
		if (anchorTraces) {
			res->anchor_trace_off = resultArray<uint64_t>(nAnchors + 1);
			res->anchor_trace_node = resultArray<int32_t>(nTrace); res->anchor_trace_offset = resultArray<uint32_t>(nTrace);
			res->anchor_trace_seqpos = resultArray<uint32_t>(nTrace); res->anchor_trace_switch = resultArray<uint8_t>(nTrace);
			res->anchor_trace_off[nAnchors] = nTrace;
		}
		res->read_chain_off = resultArray<uint64_t>(n + 1);
		res->chain = resultArray<uint32_t>(nChain);
		res->chain_score = resultArray<uint64_t>(n);
		res->read_longall_off = resultArray<uint64_t>(n + 1);
		res->read_longall_off[n] = nLong;
		res->longall_start = resultArray<uint32_t>(nLong); res->longall_end = resultArray<uint32_t>(nLong); res->longall_score = resultArray<uint32_t>(nLong);
		res->long_trace_off = resultArray<uint64_t>(nLong + 1);
		res->long_trace_off[nLong] = nLongTrace;
		res->long_trace_node = resultArray<int32_t>(nLongTrace); res->long_trace_offset = resultArray<uint32_t>(nLongTrace);
		res->long_trace_seqpos = resultArray<uint32_t>(nLongTrace); res->long_trace_switch = resultArray<uint8_t>(nLongTrace);
		res->seeds_extended_long = resultArray<uint64_t>(n);
		res->read_long_off = resultArray<uint64_t>(n + 1);
		res->read_long_off[n] = nLongSelected;
		res->long_index = resultArray<uint32_t>(nLongSelected);
		res->long_edit_distance = resultArray<int64_t>(n); res->chain_edit_distance = resultArray<int64_t>(n); res->chained_better = resultArray<uint8_t>(n);
		res->read_path_off = resultArray<uint64_t>(n + 1);
		res->read_path_off[n] = nStitched;
		res->path_node = resultArray<uint32_t>(nStitched);
		res->path_first_offset = resultArray<uint32_t>(n); res->path_last_offset = resultArray<uint32_t>(n); res->path_cells = resultArray<uint64_t>(n);
		res->read_chain_trace_off = resultArray<uint64_t>(n + 1);
		res->read_chain_trace_off[n] = nChainTrace;
		res->chain_trace_node = resultArray<int32_t>(nChainTrace); res->chain_trace_offset = resultArray<uint32_t>(nChainTrace);
		res->chain_trace_seqpos = resultArray<uint32_t>(nChainTrace); res->chain_trace_switch = resultArray<uint8_t>(nChainTrace);
		res->chain_aln_start = resultArray<uint32_t>(n); res->chain_aln_end = resultArray<uint32_t>(n);
		res->failed_assertion = resultArray<uint8_t>(n);
		res->capacity_exceeded = resultArray<uint8_t>(n);
		res->seeds_extended = resultArray<uint64_t>(n);
		res->flatten_ties = resultArray<uint32_t>(n); res->flatten_ties_long = resultArray<uint32_t>(n);
		res->read_seed_off[n] = nSeedsOut; res->read_anchor_off[n] = nAnchors; res->anchor_path_off[nAnchors] = nPath; res->read_chain_off[n] = nChain;
		pool.run(n, [&](size_t r, size_t) {
			const ReadGlue& gl = glue[r];
			res->read_seed_off[r] = seedOutBegin[r];
			if (keepSeeds) {
				uint64_t at = seedOutBegin[r];
				for (uint32_t k = 0; k < gl.nSeedsR; k++, at++) {
					const FragSeed& s = readSeeds[gl.seedBegin + k];   // fragment-pass order; pad = seedGoodness
					res->seed_node[at] = s.node; res->seed_offset[at] = s.offset; res->seed_seqpos[at] = s.seqPos; res->seed_goodness[at] = s.pad;
				}
			}
			res->read_anchor_off[r] = gl.anchorBegin;
			res->read_chain_off[r] = gl.chainBegin;
			res->chain_score[r] = chainScore[r];
			res->failed_assertion[r] = failedAssertion[r];
			res->capacity_exceeded[r] = gl.capacityExceeded ? 1 : 0;
			res->seeds_extended[r] = seedsExtended[r];
			res->seeds_extended_long[r] = seedsExtendedLong[r];
			res->flatten_ties[r] = readTies[r];                                        // (counted for every extension the reference would have run, whatever became of the read)
			res->flatten_ties_long[r] = P->long_pass ? pass.results()[r].pad : 0;
			res->read_longall_off[r] = gl.longBegin;
			res->read_path_off[r] = gl.stitchedBegin;
			res->read_long_off[r] = gl.longSelectedBegin;
			for (size_t i = 0; i < gl.longSelected.size(); i++) res->long_index[gl.longSelectedBegin + i] = gl.longSelected[i];
			res->long_edit_distance[r] = gl.longEditDistance;
			res->chain_edit_distance[r] = gl.chainEditDistance;
			// src/Aligner.cpp:901-905: the chained alignment wins when there is no whole-read alignment or its edit distance is larger
			res->chained_better[r] = gl.chainWins ? 1 : 0;
			res->read_chain_trace_off[r] = gl.chainTraceBegin;
			if (!gl.chainTraceNode.empty()) {
				memcpy(res->chain_trace_node + gl.chainTraceBegin, gl.chainTraceNode.data(), gl.chainTraceNode.size() * sizeof(int32_t));
				memcpy(res->chain_trace_offset + gl.chainTraceBegin, gl.chainTraceOffset.data(), gl.chainTraceOffset.size() * sizeof(uint32_t));
				memcpy(res->chain_trace_seqpos + gl.chainTraceBegin, gl.chainTraceSeqPos.data(), gl.chainTraceSeqPos.size() * sizeof(uint32_t));
				memcpy(res->chain_trace_switch + gl.chainTraceBegin, gl.chainTraceSwitch.data(), gl.chainTraceSwitch.size());
			}
			res->chain_aln_start[r] = gl.chainAlnStart; res->chain_aln_end[r] = gl.chainAlnEnd;
			for (size_t i = 0; i < gl.stitched.nodes.size(); i++) res->path_node[gl.stitchedBegin + i] = gl.stitched.nodes[i];
			res->path_first_offset[r] = gl.stitched.firstOffset; res->path_last_offset[r] = gl.stitched.lastOffset; res->path_cells[r] = gl.stitched.cells;
			{
				uint64_t la = gl.longBegin, lt = gl.longTraceBegin;
				for (const LongAln& al : gl.longAlns) {
					res->longall_start[la] = al.start; res->longall_end[la] = al.end; res->longall_score[la] = al.score;
					res->long_trace_off[la] = P->keep_traces ? lt : 0;
					if (P->keep_traces) for (uint32_t i = 0; i < al.traceLen; i++, lt++) {
						const LongCell& c = pass.stagedCells()[al.traceOff + i];
						res->long_trace_node[lt] = c.node; res->long_trace_offset[lt] = c.offset; res->long_trace_seqpos[lt] = c.seqPos; res->long_trace_switch[lt] = (uint8_t)c.nodeSwitch;
					}
					la++;
				}
			}
			for (uint32_t i = 0; i < chainLen[r]; i++) res->chain[gl.chainBegin + i] = chainOut[jobs[r].chainBegin + i];
			uint64_t a = gl.anchorBegin, pathAt = gl.pathBegin, traceAt = gl.traceBegin;
			if (deviceAnchors && gl.nAnchors) {   // the read's share of the dense arrays, to its place (the same place unless an earlier read of the batch lost its anchors to the whole-read pass)
				const uint64_t a0 = hAnchorOff[2 * r], w0 = hAnchorOff[2 * r + 1], cnt = gl.nAnchors;
				uint32_t* const to[9] = { res->anchor_x, res->anchor_y, res->anchor_first_node, res->anchor_first_offset, res->anchor_first_seqpos, res->anchor_last_node, res->anchor_last_offset, res->anchor_last_seqpos, (uint32_t*)res->anchor_score };
				for (int k = 0; k < 9; k++) memcpy(to[k] + gl.anchorBegin, denseWords(k) + a0, cnt * sizeof(uint32_t));
				const unsigned long long* off = densePathOff() + a0;
				for (uint64_t i = 0; i < cnt; i++) res->anchor_path_off[gl.anchorBegin + i] = off[i] - w0 + gl.pathBegin;
				memcpy(res->anchor_path + gl.pathBegin, denseWords(9) + w0, gl.nPath * sizeof(uint32_t));
			}
			if (!deviceAnchors) forEachAnchor(r, [&](uint64_t slot, uint64_t F) {
				const AnchorRec& rec = anchors[slot];
				res->anchor_x[a] = rec.x; res->anchor_y[a] = rec.y;
				res->anchor_path_off[a] = pathAt;
				for (uint32_t i = 0; i < rec.pathLen; i++) res->anchor_path[pathAt++] = pathPool[rec.pathOff + i];
				res->anchor_first_node[a] = rec.firstNode; res->anchor_first_offset[a] = rec.firstOffset; res->anchor_first_seqpos[a] = rec.firstSeqPos + frags[F].l;
				res->anchor_last_node[a] = rec.lastNode; res->anchor_last_offset[a] = rec.lastOffset; res->anchor_last_seqpos[a] = rec.lastSeqPos + frags[F].l;
				res->anchor_score[a] = rec.score;
				if (anchorTraces) {
					// merged trace in the reference's output coordinates (bigraph node id, offset in original node),
					// src/GraphAligner.h:527-565,590-608
					res->anchor_trace_off[a] = traceAt;
					const ExtResult& eb = extResults[2 * slot];
					const ExtResult& ef = extResults[2 * slot + 1];
					uint32_t p = slotSeqPos(r, slot, F) - frags[F].l;
					bool hasB = p > 0 && eb.status == EXT_OK, hasF = p < (uint32_t)P->split_len - 1 && ef.status == EXT_OK;
					if (hasB) {
						uint32_t use = hasF ? eb.traceLen - 1 : eb.traceLen;
						for (uint32_t i = 0; i < use; i++) {
							const PoolCell& c = tracePool[eb.traceOff + i];
							uint32_t off = c.offsetAndSwitch & 255u;
							auto rev = hg.GetReversePosition(hg.nodeIDs[c.node], hg.nodeOffset[c.node] + off);
							res->anchor_trace_node[traceAt] = rev.first;
							res->anchor_trace_offset[traceAt] = (uint32_t)rev.second;
							res->anchor_trace_seqpos[traceAt] = (uint32_t)((int32_t)p - 1 - c.seqPos);
							bool sw = i + 1 < eb.traceLen ? ((tracePool[eb.traceOff + i + 1].offsetAndSwitch >> 8) & 1) : false;
							res->anchor_trace_switch[traceAt] = sw ? 1 : 0;
							traceAt++;
						}
					}
					if (hasF) {
						for (uint32_t i = ef.traceLen; i-- > 0;) {
							const PoolCell& c = tracePool[ef.traceOff + i];
							uint32_t off = c.offsetAndSwitch & 255u;
							res->anchor_trace_node[traceAt] = hg.nodeIDs[c.node];
							res->anchor_trace_offset[traceAt] = (uint32_t)(hg.nodeOffset[c.node] + off);
							res->anchor_trace_seqpos[traceAt] = (uint32_t)((int32_t)p + 1 + c.seqPos);
							res->anchor_trace_switch[traceAt] = (c.offsetAndSwitch >> 8) & 1;
							traceAt++;
						}
					}
				}
				a++;
			});
		});
		output.assembleInto(res);
		res->host_us[1] = nowUs() - tAsm;
		if (sw.debugTimes) {
			// what the stream holds on the device, largest first, and how much of the pools this batch used
			std::vector<std::pair<size_t, const char*>> sizes;
			size_t total = 0;
			st->forEachDeviceBuffer([&](const char* name, size_t bytes) { if (bytes) sizes.emplace_back(bytes, name); total += bytes; });
			std::sort(sizes.begin(), sizes.end(), [](const auto& l, const auto& r) { return l.first > r.first; });
			std::string line;
			for (size_t i = 0; i < sizes.size() && i < 14; i++) { char buf[96]; snprintf(buf, sizeof buf, " %s %.2f", sizes[i].second, sizes[i].first / 1073741824.0); line += buf; }
			fprintf(stderr, "[gc mem] stream %p holds %.2f GB on the device:%s\n", (void*)st, total / 1073741824.0, line.c_str());
			fprintf(stderr, "[gc mem] %llu reads, %llu seed occurrences, %llu fragments, %llu anchor slots (%llu extensions run); trace pool %.2f of %.2f G cells, anchor path pool %.2f of %.2f G words, whole-read cells %.2f of %.2f G\n",
				(unsigned long long)n, (unsigned long long)nSeedsTotal, (unsigned long long)nFrags, (unsigned long long)nSlots, (unsigned long long)res->counters[4], hSmall[1] / 1e9, traceBudget / 1e9, hSmall[2] / 1e9, pathCapacity / 1e9,
				P->long_pass ? pass.cellsAsked() / 1e9 : 0.0, pass.cellCapacity() / 1e9);
		}
		if (sw.debugTimes) fprintf(stderr, "[gc cpu] %.0f ms up to the end of the batch (the join came at %.0f)\n", processCpuMs() - cpuCall, cpuJoined - cpuCall);
		if (sw.debugTimes) fprintf(stderr, "[gc times] batch timeline (ms from the call): whole-read pass started %.1f, joined %.1f, assembly began %.1f, done %.1f\n", (pass.startedUs() - tTotal) / 1e3, (tJoined - tTotal) / 1e3, (tAsm - tTotal) / 1e3, (nowUs() - tTotal) / 1e3);
	}
