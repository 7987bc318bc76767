// gc_batch.hip, stage by stage (r6: one file of 2 000 lines before): the chained alignments' traces, the output encoders on the device, the flat result.
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

	// ---------------- the final alignments encoded where their traces are (params->device_output; gc_output.hip): the GAF path / CIGAR text and the vg::Path bytes of
	// every alignment the reference would write for the batch (src/Aligner.cpp:901-920,1003-1023), so that no trace cell has to come down for the writers
	struct OutEntry { uint32_t read, aln; uint8_t source; };   // aln: index into the read's longAlns (source 0); source 1: the read's chained alignment, encoded by the host from its trace
	std::vector<OutEntry> outEntries;
	std::vector<uint64_t> readOutOff;
	const OutRec* hOutRecs = nullptr; const uint64_t* hOutOffsets = nullptr;
	const char* hOutPath = nullptr; const char* hOutCigar = nullptr; const uint8_t* hOutVg = nullptr;
	const uint64_t* hCorrOffsets = nullptr; const char* hCorrText = nullptr;   // (device_output & 8) the corrected pieces of the jobs: [nOutJobs + 1], letters
	uint64_t nOutJobs = 0;
	std::vector<uint64_t> outJobOfEntry;
	// Started by the whole-read pass's own thread as soon as the selection is known (the end of afterLongPass): the main thread is still in the fragment pipeline, the stitching and the
	// chain distances then, so the two passes of the encoder, their two waits and the download of the text overlap that work instead of following it (r4: with the encoder after the
	// join, every batch's latency grew by the encoder's launches waiting for wave slots among the other batches' kernels, and five streams in flight completed a batch every 255-268 ms
	// end to end against 160 for the hot path). Every read's selected alignments are encoded; a read whose chained alignment wins in the end (known only after the join) drops its pieces
	// in encodeOutput - wasted work in proportion to the winners.
	std::vector<uint64_t> readJobBegin;   // first job of every read (jobs of a read: its selected alignments sorted by alignmentStart); [n] = number of jobs
	std::vector<uint32_t> jobAln;         // the alignment (index into the read's longAlns) of every job
	void encodeOutputStart()
	{
		if (!P->device_output) return;
		const double t0 = nowUs();
		readJobBegin.assign(n + 1, 0);
		jobAln.clear();
		for (uint64_t r = 0; r < n; r++) {
			const ReadGlue& gl = glue[r];
			readJobBegin[r] = jobAln.size();
			if (gl.longFailed) continue;
			struct Item { uint32_t start; uint32_t aln; };
			std::vector<Item> items;
			for (uint32_t k : gl.longSelected) items.push_back(Item { gl.longAlns[k].start, k });
			auto byStart = [](const Item& l, const Item& rr) { return l.start < rr.start; };
			std::sort(items.begin(), items.end(), byStart);   // src/Aligner.cpp:1003
			std::sort(items.begin(), items.end(), byStart);   // :1023 (an unstable sort may move ties even in a sorted list)
			for (const Item& it : items) jobAln.push_back(it.aln);
		}
		readJobBegin[n] = jobAln.size();
		nOutJobs = jobAln.size();
		if (nOutJobs == 0) return;
		if (nOutJobs >= 0xffffffffull) throw std::runtime_error("too many alignments in one batch for the output encoder");
		OutJob* hJobsOut = st->hOutJobs.reserve<OutJob>(nOutJobs);
		const uint32_t flags = ((P->device_output & 2) ? 1u : 0u) | ((P->device_output & 3) ? 2u : 0u) | ((P->device_output & 4) ? 4u : 0u);
		for (uint64_t r = 0; r < n; r++)
			for (uint64_t k = readJobBegin[r]; k < readJobBegin[r + 1]; k++) {
				const LongAln& al = glue[r].longAlns[jobAln[k]];
				hJobsOut[k] = OutJob { al.traceOff, R->offsets[r], al.traceLen, (uint32_t)(R->offsets[r + 1] - R->offsets[r]), flags, 0 };
			}
		hipStream_t q = st->longPass.longStream;   // (the pass and its decision are done with it)
		OutJob* dJobsOut = st->outJobs.reserve<OutJob>(nOutJobs);
		OutRec* dRecs = st->outRecs.reserve<OutRec>(nOutJobs);
		uint64_t* dOffsets = st->outOffsets.reserve<uint64_t>(3 * (nOutJobs + 1));
		unsigned long long* dTotals = st->outTotals.reserve<unsigned long long>(4);
		uint32_t* dMapSizes = (P->device_output & 4) ? st->outMapSizes.reserve<uint32_t>(std::max<uint64_t>(1, pass.cellsAsked()))   /* one word per cell of the pool in use */ : nullptr;
		unsigned long long* hTotals = st->hOutTotals.reserve<unsigned long long>(4);
		HIP_CHECK(hipMemcpyAsync(dJobsOut, hJobsOut, nOutJobs * sizeof(OutJob), hipMemcpyHostToDevice, q));
		hipEvent_t timed[6] = {};   // GC_DEBUG_TIMES: device time of the encoder's and the corrected reads' kernels, each pass between events of its own
		if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
		auto mark = [&](int k) { if (timed[k]) HIP_CHECK(hipEventRecord(timed[k], q)); };
		mark(0);
		launchOutCount(q, G->dev, G->devNames, G->devIupac, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), R->devBases, dRecs, dOffsets, dMapSizes, dTotals);
		mark(1);
		HIP_CHECK(hipMemcpyAsync(hTotals, dTotals, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
		// corrected reads (device_output & 8; gc_corrected.hip): their own kernels behind the encoder's on the same stream, their count and text beside the encoder's
		const bool corrected = (P->device_output & 8) != 0;
		uint32_t* dCorrLens = nullptr; uint64_t* dCorrOffsets = nullptr; unsigned long long* hCorrTotal = nullptr;
		if (corrected) {
			dCorrLens = st->corrLens.reserve<uint32_t>(nOutJobs);
			dCorrOffsets = st->corrOffsets.reserve<uint64_t>(nOutJobs + 1);
			unsigned long long* dCorrTotal = st->corrTotal.reserve<unsigned long long>(1);
			hCorrTotal = st->hCorrTotal.reserve<unsigned long long>(1);
			launchCorrectedCount(q, G->dev, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), dCorrLens, dCorrOffsets, dCorrTotal);
			HIP_CHECK(hipMemcpyAsync(hCorrTotal, dCorrTotal, sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
		}
		mark(2);
		syncStream(q);
		const uint64_t pathBytes = hTotals[0], cigarBytes = hTotals[1], vgBytes = hTotals[2];
		char* dPath = st->outPathText.reserve<char>(pathBytes + 1);
		char* dCigar = st->outCigarText.reserve<char>(cigarBytes + 1);
		uint8_t* dVg = st->outVgBytes.reserve<uint8_t>(vgBytes + 1);
		mark(3);
		launchOutWrite(q, G->dev, G->devNames, G->devIupac, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), R->devBases, dRecs, dOffsets, dMapSizes, dPath, dCigar, dVg);
		mark(4);
		OutRec* recs = st->hOutRecs.reserve<OutRec>(nOutJobs);
		uint64_t* offs = st->hOutOffsets.reserve<uint64_t>(3 * (nOutJobs + 1));
		char* pathText = st->hOutPathText.reserve<char>(pathBytes + 1);
		char* cigarText = st->hOutCigarText.reserve<char>(cigarBytes + 1);
		uint8_t* vg = st->hOutVgBytes.reserve<uint8_t>(vgBytes + 1);
		HIP_CHECK(hipMemcpyAsync(recs, dRecs, nOutJobs * sizeof(OutRec), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(offs, dOffsets, 3 * (nOutJobs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
		if (pathBytes) HIP_CHECK(hipMemcpyAsync(pathText, dPath, pathBytes, hipMemcpyDeviceToHost, q));
		if (cigarBytes) HIP_CHECK(hipMemcpyAsync(cigarText, dCigar, cigarBytes, hipMemcpyDeviceToHost, q));
		if (vgBytes) HIP_CHECK(hipMemcpyAsync(vg, dVg, vgBytes, hipMemcpyDeviceToHost, q));
		uint64_t corrBytes = 0;
		uint32_t* corrLens = nullptr;
		if (corrected) {
			corrBytes = *hCorrTotal;
			char* dCorrText = st->corrText.reserve<char>(corrBytes + 1);
			launchCorrectedWrite(q, G->dev, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), dCorrLens, dCorrOffsets, dCorrText);
			mark(5);
			corrLens = st->hCorrLens.reserve<uint32_t>(nOutJobs);
			uint64_t* corrOffs = st->hCorrOffsets.reserve<uint64_t>(nOutJobs + 1);
			char* corrText = st->hCorrText.reserve<char>(corrBytes + 1);
			HIP_CHECK(hipMemcpyAsync(corrLens, dCorrLens, nOutJobs * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipMemcpyAsync(corrOffs, dCorrOffsets, (nOutJobs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
			if (corrBytes) HIP_CHECK(hipMemcpyAsync(corrText, dCorrText, corrBytes, hipMemcpyDeviceToHost, q));
			hCorrOffsets = corrOffs; hCorrText = corrText;
		}
		syncStream(q);
		if (corrected) for (uint64_t k = 0; k < nOutJobs; k++) if (corrLens[k] == 0xffffffffu) throw std::runtime_error("internal: the corrected-read kernel's two passes disagree on an alignment's size");
		for (uint64_t k = 0; k < nOutJobs; k++) if (recs[k].steps == 0xffffffffu) throw std::runtime_error("internal: the output encoder's two passes disagree on an alignment's size");
		hOutRecs = recs; hOutOffsets = offs; hOutPath = pathText; hOutCigar = cigarText; hOutVg = vg;
		if (sw.debugTimes) fprintf(stderr, "[gc times] output encoding on the device: %llu alignments, %.1f MB of path text, %.1f MB of CIGAR, %.1f MB of vg::Path bytes, %.1f ms (on the whole-read pass's thread, beside the fragment pipeline)\n",
			(unsigned long long)nOutJobs, pathBytes / 1e6, cigarBytes / 1e6, vgBytes / 1e6, (nowUs() - t0) / 1e3);
		if (timed[0]) {
			auto between = [&](int a, int b) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, timed[a], timed[b])); return (double)ms; };
			const double encodeMs = between(0, 1) + between(3, 4), correctedMs = corrected ? between(1, 2) + between(4, 5) : 0.0;
			for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
			fprintf(stderr, "[gc times] output kernels on the device: k_out_encode (both passes, k_out_place) %.3f ms; corrected reads (k_corr_walk both passes, k_corr_place) %.3f ms, %.1f MB of letters down\n",
				encodeMs, correctedMs, corrBytes / 1e6);
		}
	}

	// After the decision: which of the encoded alignments are the batch's output, in the reference's order
	void encodeOutput()
	{
		if (!P->device_output) return;
		readOutOff.assign(n + 1, 0);
		outEntries.clear();
		outJobOfEntry.clear();
		for (uint64_t r = 0; r < n; r++) {
			const ReadGlue& gl = glue[r];
			readOutOff[r] = outEntries.size();
			if (gl.longFailed) continue;
			if (gl.chainWins) { outEntries.push_back(OutEntry { (uint32_t)r, 0, 1 }); outJobOfEntry.push_back(~0ull); continue; }
			for (uint64_t k = readJobBegin[r]; k < readJobBegin[r + 1]; k++) { outEntries.push_back(OutEntry { (uint32_t)r, jobAln[k], 0 }); outJobOfEntry.push_back(k); }
		}
		readOutOff[n] = outEntries.size();
		if (st->coverage) countCoverage();
	}

	// gc_stream_set_coverage: the batch's output entries - exactly the alignments the writers will print - are counted into the handle (gc_coverage.hip). Here and not beside the
	// encoder: the encoder runs before the chained-versus-whole-read decision and drops the losers' pieces afterwards, and a count cannot be dropped. Entries of source 0 are
	// read where they lie, in the cell pool (still resident: nothing reserves it again before the next batch), under a keep byte per encoder job; the chained winners' traces
	// exist only on the host (chain_trace_*: edlib's path walked, or the fast mode's stitched cells) and go up for the same kernel. The stream is waited for: a finished batch
	// is a counted batch.
	void countCoverage()
	{
		gc_coverage* cov = st->coverage;
		const double t0 = nowUs();
		hipEvent_t timed[2] = {};
		if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
		if (timed[0]) HIP_CHECK(hipEventRecord(timed[0], stream));
		uint64_t nKept = 0, nWinners = 0, winnerCells = 0;
		if (nOutJobs) {
			uint8_t* hKeep = st->hCovKeep.reserve<uint8_t>(nOutJobs);
			memset(hKeep, 0, nOutJobs);
			for (uint64_t k : outJobOfEntry) if (k != ~0ull) { hKeep[k] = 1; nKept++; }
			if (nKept) {
				uint8_t* dKeep = st->covKeep.reserve<uint8_t>(nOutJobs);
				HIP_CHECK(hipMemcpyAsync(dKeep, hKeep, nOutJobs, hipMemcpyHostToDevice, stream));
				launchCoverageAdd(stream, cov->dev, cov->links, (const OutJob*)st->outJobs.ptr, (uint32_t)nOutJobs, dKeep, pass.deviceCells(), cov->dBases, cov->dDepth, cov->dBad);
			}
		}
		for (const OutEntry& en : outEntries) if (en.source == 1) { nWinners++; winnerCells += glue[en.read].chainTraceNode.size(); }
		if (nWinners) {
			if (nWinners >= 0xffffffffull) throw std::runtime_error("too many chained alignments in one batch for the coverage kernel");
			LongCell* hCells = st->hCovCells.reserve<LongCell>(winnerCells);
			OutJob* hJobsCov = st->hCovJobs.reserve<OutJob>(nWinners);
			uint64_t at = 0, w = 0;
			for (const OutEntry& en : outEntries) {
				if (en.source != 1) continue;
				const ReadGlue& gl = glue[en.read];
				const size_t cells = gl.chainTraceNode.size();
				if (cells == 0) throw std::runtime_error("coverage: a chained alignment won and the batch holds no trace for it (chain_traces == 0?)");
				hJobsCov[w++] = OutJob { at, 0, (uint32_t)cells, 0, 0, 0 };
				for (size_t i = 0; i < cells; i++) hCells[at++] = LongCell { gl.chainTraceNode[i], gl.chainTraceOffset[i], gl.chainTraceSeqPos[i], gl.chainTraceSwitch[i] };
			}
			LongCell* dCells = st->covCells.reserve<LongCell>(winnerCells);
			OutJob* dJobsCov = st->covJobs.reserve<OutJob>(nWinners);
			HIP_CHECK(hipMemcpyAsync(dCells, hCells, winnerCells * sizeof(LongCell), hipMemcpyHostToDevice, stream));
			HIP_CHECK(hipMemcpyAsync(dJobsCov, hJobsCov, nWinners * sizeof(OutJob), hipMemcpyHostToDevice, stream));
			launchCoverageAdd(stream, cov->dev, cov->links, dJobsCov, (uint32_t)nWinners, nullptr, dCells, cov->dBases, cov->dDepth, cov->dBad);
		}
		if (timed[1]) HIP_CHECK(hipEventRecord(timed[1], stream));
		HIP_CHECK(hipGetLastError());
		syncStream(stream);
		if (timed[0]) {
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, timed[0], timed[1]));
			for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
			fprintf(stderr, "[gc times] coverage: k_cov_add over %llu alignments in the cell pool and %llu chained winners (%llu cells up), %.3f ms on the device, %.1f ms in all; per-base depth %s, links %s\n",
				(unsigned long long)nKept, (unsigned long long)nWinners, (unsigned long long)winnerCells, ms, (nowUs() - t0) / 1e3, cov->dDepth ? "on" : "off", cov->hasLinks ? "on" : "off");
		}
	}

	void assembleOutput()   // the pieces into the result (entries of chained winners stay empty: source 1)
	{
		res->device_output = P->device_output;
		if (!P->device_output) return;
		const uint64_t nOut = outEntries.size();
		res->read_out_off = resultArray<uint64_t>(n + 1);
		memcpy(res->read_out_off, readOutOff.data(), (n + 1) * sizeof(uint64_t));
		res->out_source = resultArray<uint8_t>(nOut);
		res->out_numbers = resultArray<uint64_t>(12 * nOut);
		res->out_path_off = resultArray<uint64_t>(nOut + 1); res->out_cigar_off = resultArray<uint64_t>(nOut + 1); res->out_vg_off = resultArray<uint64_t>(nOut + 1);
		const uint64_t stride = nOutJobs + 1;
		// where every entry's pieces go: the kept jobs' bytes back to back (all of them, in order, unless chained alignments won)
		uint64_t pathBytes = 0, cigarBytes = 0, vgBytes = 0;
		for (uint64_t e = 0; e < nOut; e++) {
			res->out_path_off[e] = pathBytes; res->out_cigar_off[e] = cigarBytes; res->out_vg_off[e] = vgBytes;
			const uint64_t k = outJobOfEntry[e];
			if (k == ~0ull) continue;
			pathBytes += hOutOffsets[k + 1] - hOutOffsets[k]; cigarBytes += hOutOffsets[stride + k + 1] - hOutOffsets[stride + k]; vgBytes += hOutOffsets[2 * stride + k + 1] - hOutOffsets[2 * stride + k];
		}
		res->out_path_off[nOut] = pathBytes; res->out_cigar_off[nOut] = cigarBytes; res->out_vg_off[nOut] = vgBytes;
		res->out_path_text = resultArray<char>(pathBytes + 1); res->out_cigar_text = resultArray<char>(cigarBytes + 1); res->out_vg_path = resultArray<uint8_t>(vgBytes + 1);
		bool allKept = nOut == nOutJobs;   // no chained winner: the device's blobs are the result's, job k is entry k
		for (uint64_t e = 0; e < nOut && allKept; e++) allKept = outJobOfEntry[e] == e;   // (a winner's one entry can stand where a read's one dropped job was: the counts alone do not tell)
		const size_t parts = 16;
		if (allKept) pool.run(3 * parts, [&](size_t i, size_t) {
			const size_t which = i / parts, part = i % parts;
			const uint64_t total = which == 0 ? pathBytes : which == 1 ? cigarBytes : vgBytes;
			const char* src = which == 0 ? hOutPath : which == 1 ? hOutCigar : (const char*)hOutVg;
			char* dst = which == 0 ? res->out_path_text : which == 1 ? res->out_cigar_text : (char*)res->out_vg_path;
			const uint64_t b = total * part / parts, e = total * (part + 1) / parts;
			if (e > b) memcpy(dst + b, src + b, e - b);
		});
		else pool.run(nOut, [&](size_t e, size_t) {
			const uint64_t k = outJobOfEntry[e];
			if (k == ~0ull) return;
			memcpy(res->out_path_text + res->out_path_off[e], hOutPath + hOutOffsets[k], hOutOffsets[k + 1] - hOutOffsets[k]);
			memcpy(res->out_cigar_text + res->out_cigar_off[e], hOutCigar + hOutOffsets[stride + k], hOutOffsets[stride + k + 1] - hOutOffsets[stride + k]);
			memcpy(res->out_vg_path + res->out_vg_off[e], hOutVg + hOutOffsets[2 * stride + k], hOutOffsets[2 * stride + k + 1] - hOutOffsets[2 * stride + k]);
		});
		res->out_path_text[pathBytes] = 0; res->out_cigar_text[cigarBytes] = 0;
		if (P->device_output & 8) {   // the corrected pieces, compacted like the other three (entries of chained winners stay empty: the host spells them from chain_trace_*)
			res->out_corrected_off = resultArray<uint64_t>(nOut + 1);
			uint64_t corrBytes = 0;
			for (uint64_t e = 0; e < nOut; e++) {
				res->out_corrected_off[e] = corrBytes;
				const uint64_t k = outJobOfEntry[e];
				if (k != ~0ull) corrBytes += hCorrOffsets[k + 1] - hCorrOffsets[k];
			}
			res->out_corrected_off[nOut] = corrBytes;
			res->out_corrected_text = resultArray<char>(corrBytes + 1);
			if (allKept) pool.run(parts, [&](size_t part, size_t) {
				const uint64_t b = corrBytes * part / parts, e = corrBytes * (part + 1) / parts;
				if (e > b) memcpy(res->out_corrected_text + b, hCorrText + b, e - b);
			});
			else pool.run(nOut, [&](size_t e, size_t) {
				const uint64_t k = outJobOfEntry[e];
				if (k != ~0ull) memcpy(res->out_corrected_text + res->out_corrected_off[e], hCorrText + hCorrOffsets[k], hCorrOffsets[k + 1] - hCorrOffsets[k]);
			});
			res->out_corrected_text[corrBytes] = 0;
		}
		for (uint64_t e = 0; e < nOut; e++) {
			const OutEntry& en = outEntries[e];
			res->out_source[e] = en.source;
			uint64_t* num = res->out_numbers + 12 * e;
			if (en.source == 0) {
				const OutRec& rec = hOutRecs[outJobOfEntry[e]];
				const LongAln& al = glue[en.read].longAlns[en.aln];
				num[0] = rec.nodePathLen; num[1] = rec.nodePathStart; num[2] = rec.nodePathEnd; num[3] = rec.matches; num[4] = rec.mismatches; num[5] = rec.insertions; num[6] = rec.deletions;
				num[7] = al.traceLen; num[8] = al.start; num[9] = al.end; num[10] = rec.steps; num[11] = al.score;
			} else for (int i = 0; i < 12; i++) num[i] = 0;
		}
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
		assembleOutput();
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
